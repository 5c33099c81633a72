// tile_order.hpp -- the host-built, XCD-aware tile order of the large GEMM launches (gemm.hip): which tiles a launch needs and
// in which order its workgroups take them.  Pure list building, no HIP calls: gemm.hip uploads and caches the table, and
// test_aids/tile_order_host.cpp builds it on the CPU (tests/test_tile_order_host.py).
//
// Workgroup b runs on XCD b % 8 and the workgroups of one XCD start in the order of b / 8.  The needed tiles are put
// in ONE sequence -- supertiles of 64 x 8 tiles (rows x columns) in row-major order, each walked row by row -- and the
// sequence is cut into eight contiguous pieces of equal length, one per XCD.  The ~110 workgroups resident on an XCD then
// share 8 B-panels (kept in its L2 for 64 tile rows) and each A-panel eight times, and every XCD gets the same number of
// tiles to within one.  Measured on a 7168-row rank-384 update (scratch/pmc_order.sh, scratch/gemm_time.py): 8 x 8
// supertiles dealt round robin (round 1) 637 MB fetched / 412-417 us, the same cut evenly 674 MB / 402 us (the XCDs'
// lists differed by up to one supertile = 8 % of a small launch: 4096 rows 157 -> 145 us), 64 x 8 cut evenly 503 MB /
// 404 us, 16 x 16 846 MB (the streamed C tiles leave the panels well under the L2's 4 MB).  GPT_TILE_ORDER="rows,cols,mode"
// overrides (mode 0 = round-robin deal).  Slots past an XCD's list hold (-1, -1).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct TileIJ { int x, y; };      // (tile row, tile column): the layout of the device table's int2 entries

// tri == 2: staircase.  Column segment q = j / seg_t starts (its diagonal block) at tile row q * rss_t; tile (i, j) is
// needed iff i >= q * rss_t + (j - q * seg_t).
// tri == 3: grid staircase (2-D block-cyclic layout, gptools_amd/dist.py GridLML).  Column segment q is local block column q of
// the update, global block column J = J0 + q * num; the local block rows hold the global block rows I = pr + li * den.  Its
// first needed block row is the first I >= J:  rs(q) = ceil((off + q * num) / den) - base  with off = J0 - pr and base = the
// local index of the update's first block row.  Below that row the segment is a full rectangle; the first block itself is a
// DIAGONAL block of the matrix iff (off + q * num) is a multiple of den, and then only its lower tiles are needed.
struct GridStair { int64_t off = 0, num = 0, den = 1, base = 0; };
// live_tm: tile rows from this one on hold no row the result needs (the padding rows of a fit's augmented factor, see
// launch_gemm_nt) and are not enumerated; ntm = all rows
static inline bool tile_needed(int tri, int64_t i, int64_t j, int64_t seg_t, int64_t rss_t, const GridStair &g, int64_t live_tm)
{
    if (i >= live_tm) return false;
    if (tri == 1) return j <= i;
    if (tri == 2) {
        const int64_t q = j / seg_t;
        return i >= q * rss_t + (j - q * seg_t);
    }
    if (tri == 3) {
        const int64_t q = j / seg_t, v = g.off + q * g.num;
        const int64_t i0 = ((v + g.den - 1) / g.den - g.base) * seg_t;
        if (i < i0) return false;
        if (v % g.den == 0 && i < i0 + seg_t) return (i - i0) >= (j - q * seg_t);
        return true;
    }
    return true;
}

struct TileTable {
    std::vector<TileIJ> flat;      // entry l * 8 + x: the l-th tile of XCD x, or (-1, -1) past the end of that XCD's list
    int64_t ntiles = 0;            // entries that hold a tile
    int64_t nedge = 0;             // ... of which in the first edge_cols tile columns (they come first in every XCD's list)
};

// sgm x sgn: the supertile (tiles); mode 0: whole supertiles dealt round robin (only without edge_cols), else cut evenly
static inline TileTable build_tile_table(int64_t ntm, int64_t ntn, int tri, int64_t seg_t, int64_t rss_t, int64_t edge_cols,
                                         const GridStair &gs, int64_t live_tm, int sgm, int sgn, int mode)
{
    std::vector<std::vector<TileIJ>> per(8);
    std::vector<TileIJ> seq, sequ;          // sequ: the tiles of the first edge_cols columns (they go first on every XCD)
    const int64_t sm = (ntm + sgm - 1) / sgm, sn = (ntn + sgn - 1) / sgn;
    int64_t sidx = 0;
    for (int64_t si = 0; si < sm; si++)
        for (int64_t sj = 0; sj < sn; sj++) {
            std::vector<TileIJ> &dst = (mode || edge_cols > 0) ? seq : per[sidx % 8];
            bool any = false;
            for (int64_t i = si * sgm; i < (si + 1) * sgm && i < ntm; i++)
                for (int64_t j = sj * sgn; j < (sj + 1) * sgn && j < ntn; j++) {
                    if (!tile_needed(tri, i, j, seg_t, rss_t, gs, live_tm)) continue;
                    (j < edge_cols ? sequ : dst).push_back(TileIJ{(int)i, (int)j});
                    any = true;
                }
            if (any) sidx++;
        }
    if (mode || edge_cols > 0) {
        for (const std::vector<TileIJ> *sq : {&sequ, &seq}) {
            const size_t T = sq->size(), q = T / 8, r = T % 8;
            size_t at = 0;
            for (int x = 0; x < 8; x++) {
                const size_t len = q + ((size_t)x < r ? 1 : 0);
                per[x].insert(per[x].end(), sq->begin() + at, sq->begin() + at + len);
                at += len;
            }
        }
    }
    size_t mx = 0;
    for (auto &v : per) mx = v.size() > mx ? v.size() : mx;
    TileTable t;
    t.flat.assign(mx * 8, TileIJ{-1, -1});
    for (int x = 0; x < 8; x++)
        for (size_t l = 0; l < per[x].size(); l++) t.flat[l * 8 + x] = per[x][l];
    t.nedge = (int64_t)sequ.size();
    for (auto &v : per) t.ntiles += (int64_t)v.size();
    return t;
}
