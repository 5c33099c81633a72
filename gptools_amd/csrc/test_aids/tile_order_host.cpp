// tile_order_host.cpp -- test aid (not part of the product library): the order-table builder of the large GEMM launches
// (../tile_order.hpp) on the CPU, tests/test_tile_order_host.py.  A stand-alone program, built with the address and undefined-
// behaviour sanitizers (Makefile: tile_order_host); exit status 0 and a line "ok <cases>" when every property holds, otherwise one line
// per violated property and status 1.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "../tile_order.hpp"

// ---- the builder as it stood before the live-row limit, verbatim (int2 / make_int2 restated for the host) --------------------
struct int2 { int x, y; };
static inline int2 make_int2(int x, int y) { return int2{x, y}; }
static inline bool tile_needed_old(int tri, int64_t i, int64_t j, int64_t seg_t, int64_t rss_t, const GridStair &g = GridStair())
{
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
static std::vector<int2> old_table(int64_t ntm, int64_t ntn, int tri, int64_t seg_t, int64_t rss_t, int64_t edge_cols, const GridStair &gs,
                                   int sgm, int sgn, int mode, int64_t *ntiles, int64_t *nedge)
{
    std::vector<std::vector<int2>> per(8);
    std::vector<int2> seq, sequ;          // sequ: the tiles of the first edge_cols columns (they go first on every XCD)
    const int64_t sm = (ntm + sgm - 1) / sgm, sn = (ntn + sgn - 1) / sgn;
    int64_t sidx = 0;
    for (int64_t si = 0; si < sm; si++)
        for (int64_t sj = 0; sj < sn; sj++) {
            std::vector<int2> &dst = (mode || edge_cols > 0) ? seq : per[sidx % 8];
            bool any = false;
            for (int64_t i = si * sgm; i < (si + 1) * sgm && i < ntm; i++)
                for (int64_t j = sj * sgn; j < (sj + 1) * sgn && j < ntn; j++) {
                    if (!tile_needed_old(tri, i, j, seg_t, rss_t, gs)) continue;
                    (j < edge_cols ? sequ : dst).push_back(make_int2((int)i, (int)j));
                    any = true;
                }
            if (any) sidx++;
        }
    if (mode || edge_cols > 0) {
        for (const std::vector<int2> *sq : {&sequ, &seq}) {
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
    std::vector<int2> flat(mx * 8, make_int2(-1, -1));
    for (int x = 0; x < 8; x++)
        for (size_t l = 0; l < per[x].size(); l++) flat[l * 8 + x] = per[x][l];
    *nedge = (int64_t)sequ.size();
    *ntiles = 0;
    for (auto &v : per) *ntiles += (int64_t)v.size();
    return flat;
}

static int g_bad = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            g_bad++;                      \
            printf("FAIL " __VA_ARGS__);  \
            printf("\n");                 \
        }                                 \
    } while (0)

// one table of a tri launch: ntm x ntn tiles, the tile rows from live_tm on left out, the first edge_cols columns urgent
static void check_case(int64_t ntm, int64_t ntn, int64_t live_tm, int64_t edge_cols, int mode)
{
    const int sgm = 64, sgn = 8;
    const TileTable t = build_tile_table(ntm, ntn, 1, 0, 0, edge_cols, GridStair(), live_tm, sgm, sgn, mode);
    char id[128];
    snprintf(id, sizeof(id), "ntm=%lld ntn=%lld live=%lld edge_cols=%lld mode=%d", (long long)ntm, (long long)ntn, (long long)live_tm,
             (long long)edge_cols, mode);
    EXPECT(t.flat.size() % 8 == 0, "%s: table length %zu", id, t.flat.size());
    const size_t rows = t.flat.size() / 8;
    // every needed tile exactly once, none that starts at or beyond the limit
    std::set<std::pair<int, int>> seen;
    int64_t want = 0, want_edge = 0;
    for (int64_t i = 0; i < ntm && i < live_tm; i++)
        for (int64_t j = 0; j < ntn && j <= i; j++) {
            want++;
            if (j < edge_cols) want_edge++;
        }
    size_t len[8], ulen[8];
    for (int x = 0; x < 8; x++) {
        len[x] = ulen[x] = 0;
        bool ended = false, rest = false;
        for (size_t l = 0; l < rows; l++) {
            const TileIJ e = t.flat[l * 8 + x];
            if (e.x < 0) {
                EXPECT(e.x == -1 && e.y == -1, "%s: XCD %d slot %zu holds (%d, %d)", id, x, l, e.x, e.y);
                ended = true;
                continue;
            }
            EXPECT(!ended, "%s: XCD %d has a tile behind an empty slot (%zu)", id, x, l);
            EXPECT(e.x < live_tm, "%s: tile row %d starts at or beyond the limit", id, e.x);
            EXPECT(e.x < ntm && e.y >= 0 && e.y < ntn && e.y <= e.x, "%s: tile (%d, %d) is not in the launch", id, e.x, e.y);
            EXPECT(seen.insert(std::make_pair(e.x, e.y)).second, "%s: tile (%d, %d) twice", id, e.x, e.y);
            // the urgent tiles come first in every XCD's list
            if (e.y < edge_cols) {
                EXPECT(!rest, "%s: XCD %d: urgent tile (%d, %d) behind a tile of the rest", id, x, e.x, e.y);
                ulen[x]++;
            } else {
                rest = true;
            }
            len[x]++;
        }
    }
    EXPECT((int64_t)seen.size() == want, "%s: %zu tiles, %lld needed", id, seen.size(), (long long)want);
    EXPECT(t.ntiles == want, "%s: ntiles %lld, %lld needed", id, (long long)t.ntiles, (long long)want);
    EXPECT(t.nedge == want_edge, "%s: nedge %lld, %lld urgent tiles", id, (long long)t.nedge, (long long)want_edge);
    // the eight lists differ in length by at most one (the even cut; mode 0 deals whole supertiles and promises nothing).  With urgent
    // columns the urgent tiles and the rest are TWO sequences, each cut evenly with its remainder on the first XCDs: each part then
    // differs by at most one over the XCDs and the whole lists by at most two -- that is the table as it has always been built (it
    // is compared with the old builder below), so a bound of one on the whole list holds only without urgent columns.
    if (mode || edge_cols > 0) {
        size_t lo = len[0], hi = len[0], ulo = ulen[0], uhi = ulen[0], rlo = len[0] - ulen[0], rhi = rlo;
        for (int x = 1; x < 8; x++) {
            const size_t r = len[x] - ulen[x];
            lo = len[x] < lo ? len[x] : lo, hi = len[x] > hi ? len[x] : hi;
            ulo = ulen[x] < ulo ? ulen[x] : ulo, uhi = ulen[x] > uhi ? ulen[x] : uhi;
            rlo = r < rlo ? r : rlo, rhi = r > rhi ? r : rhi;
        }
        EXPECT(uhi - ulo <= 1, "%s: urgent parts of %zu ... %zu tiles", id, ulo, uhi);
        EXPECT(rhi - rlo <= 1, "%s: rest parts of %zu ... %zu tiles", id, rlo, rhi);
        EXPECT(hi - lo <= (edge_cols > 0 ? 2u : 1u), "%s: lists of %zu ... %zu tiles", id, lo, hi);
        EXPECT(hi == rows, "%s: %zu table rows for lists of at most %zu", id, rows, hi);
    }
    // with the limit at "all rows" the table is the one the old builder makes
    if (live_tm >= ntm) {
        int64_t nt = 0, ne = 0;
        const std::vector<int2> ref = old_table(ntm, ntn, 1, 0, 0, edge_cols, GridStair(), sgm, sgn, mode, &nt, &ne);
        bool same = ref.size() == t.flat.size() && nt == t.ntiles && ne == t.nedge;
        for (size_t l = 0; same && l < ref.size(); l++) same = ref[l].x == t.flat[l].x && ref[l].y == t.flat[l].y;
        EXPECT(same, "%s: differs from the old builder's table", id);
    }
}

// the staircase tables (tri 2 / 3) take no limit: unchanged from the old builder
static void check_stairs()
{
    GridStair g;
    g.off = 1, g.num = 2, g.den = 3, g.base = 0;
    struct { int tri; int64_t ntm, ntn, seg_t, rss_t; } cs[] = {{0, 40, 12, 0, 0}, {2, 48, 24, 8, 8}, {2, 40, 16, 4, 12}, {3, 48, 24, 8, 0}};
    for (auto &c : cs) {
        const GridStair gs = c.tri == 3 ? g : GridStair();
        int64_t nt = 0, ne = 0;
        const std::vector<int2> ref = old_table(c.ntm, c.ntn, c.tri, c.seg_t, c.rss_t, 0, gs, 64, 8, 1, &nt, &ne);
        const TileTable t = build_tile_table(c.ntm, c.ntn, c.tri, c.seg_t, c.rss_t, 0, gs, c.ntm, 64, 8, 1);
        bool same = ref.size() == t.flat.size() && nt == t.ntiles && ne == t.nedge;
        for (size_t l = 0; same && l < ref.size(); l++) same = ref[l].x == t.flat[l].x && ref[l].y == t.flat[l].y;
        EXPECT(same, "tri=%d ntm=%lld ntn=%lld: differs from the old builder's table", c.tri, (long long)c.ntm, (long long)c.ntn);
    }
}

int main()
{
    int cases = 0;
    const int64_t sizes[] = {8, 33, 36, 82, 124};
    const int64_t edges[] = {0, 4, 6};
    for (int64_t nt : sizes)
        for (int64_t cut = 0; cut <= 2; cut++)
            for (int64_t ec : edges)
                for (int mode = 1; mode >= (ec > 0 ? 1 : 0); mode--) {
                    check_case(nt, nt, nt - cut, ec, mode);
                    cases++;
                }
    // more rows than columns (an urgent-only launch), and a limit that ends the launch inside its triangle
    for (int64_t cut = 0; cut <= 2; cut++) {
        check_case(124, 6, 124 - cut, 0, 1);
        check_case(116, 100, 116 - cut, 6, 1);
        check_case(40, 40, 30 - cut, 4, 1);
        cases += 3;
    }
    check_stairs();
    if (g_bad) {
        printf("%d properties violated\n", g_bad);
        return 1;
    }
    printf("ok %d\n", cases);
    return 0;
}
