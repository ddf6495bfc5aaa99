// Lane tables of the resident B-grid kernel's rim-wave schedule: see rim_plan.h.  Plain host code.
#include "rim_plan.h"

#include <algorithm>

namespace rim_plan {

namespace {

// the owned U-cells that read T-cell pos and are not in L_U yet
int missing_ucells(int pos, const uint8_t *uown, const bool *in_lu, int *which)
{
    const int r = pos / W, c = pos % W;
    int n = 0;
    for (int dr = 0; dr < 2; ++dr)
        for (int dc = 0; dc < 2; ++dc) {
            const int ur = r - dr, uc = c - dc;
            if (ur < 0 || uc < 0 || ur > W - 2 || uc > W - 2) continue;
            const int u = ur * W + uc;
            if (uown[u] && !in_lu[u]) which[n++] = u;
        }
    return n;
}

}  // namespace

void tile(const uint8_t *cls, const uint8_t *ice, const uint8_t *uown, const uint8_t *upub, Tile &o)
{
    bool on[NPOS], in_lt[NPOS], in_lu[NPOS];
    int n = 0, n_lt = 0, n_lu = 0;
    for (int pos = 0; pos < NPOS; ++pos) {
        on[pos] = cls[pos] != 0 && ice[pos];
        in_lt[pos] = on[pos] && cls[pos] == 2;
        in_lu[pos] = uown[pos] && upub[pos];
        n += on[pos];
        n_lt += in_lt[pos];
        n_lu += in_lu[pos];
    }
    int add[4];
    for (int pos = 0; pos < NPOS; ++pos)
        if (in_lt[pos]) {
            const int m = missing_ucells(pos, uown, in_lu, add);
            for (int q = 0; q < m; ++q) in_lu[add[q]] = true;
            n_lu += m;
        }
    o.ok = n_lt <= 64 && n_lu <= 64;
    const int packed = (n + 63) / 64;
    o.nact_packed = packed;
    // fill-up: the ice-first packing puts n - 64 (packed - 1) cells into the first chunk
    const int need = n > 0 ? n - 64 * (packed - 1) : 0;
    const int corners[4] = {1 * W + 1, 1 * W + (W - 2), (W - 2) * W + 1, (W - 2) * W + (W - 2)};
    while (o.ok && n_lt < need) {
        int best = -1, best_m = 5;
        for (int q = 0; q < 4 && best < 0; ++q) {      // a depth-1 corner cell costs one lane of L_U
            const int pos = corners[q];
            if (on[pos] && !in_lt[pos] && n_lu + missing_ucells(pos, uown, in_lu, add) <= 64) best = pos;
        }
        if (best < 0)
            for (int pos = 0; pos < NPOS; ++pos) {      // otherwise the cell that costs the fewest
                if (!on[pos] || in_lt[pos]) continue;
                const int m = missing_ucells(pos, uown, in_lu, add);
                if (n_lu + m <= 64 && m < best_m) { best = pos; best_m = m; }
            }
        if (best < 0) break;
        const int m = missing_ucells(best, uown, in_lu, add);
        for (int q = 0; q < m; ++q) in_lu[add[q]] = true;
        n_lu += m;
        in_lt[best] = true;
        ++n_lt;
    }
    const int rest = n - n_lt;
    if (rest > 3 * 64) o.ok = false;          // an ice cell would have to sit in chunk 0 without being in L_T
    o.n_lt = n_lt;
    o.n_lu = n_lu;
    o.nact = n > 0 ? 1 + (rest + 63) / 64 : 0;
    // lanes: chunk 0 = L_T, padded with positions without ice; then the other ice cells; then the rest
    int k = 0;
    bool placed[NPOS];
    std::fill(placed, placed + NPOS, false);
    auto put = [&](int pos) { o.perm[k++] = (uint8_t)pos; placed[pos] = true; };
    for (int pos = 0; pos < NPOS; ++pos)
        if (in_lt[pos]) put(pos);
    for (int pos = 0; pos < NPOS && k < 64; ++pos)
        if (!on[pos]) put(pos);
    for (int pos = 0; pos < NPOS && k < 64; ++pos)      // (only where the tile is not ok: chunk 0 takes what is left)
        if (!placed[pos]) put(pos);
    for (int pos = 0; pos < NPOS; ++pos)
        if (on[pos] && !placed[pos]) put(pos);
    for (int pos = 0; pos < NPOS; ++pos)
        if (!placed[pos]) put(pos);
    std::fill(o.uperm, o.uperm + NPOS, (uint8_t)NONE);
    int ku = 0;
    for (int pos = 0; pos < NPOS && ku < 64; ++pos)
        if (in_lu[pos]) o.uperm[ku++] = (uint8_t)pos;
    for (int lane = 64; lane < NPOS; ++lane) {
        const int pos = o.perm[lane];
        if (uown[pos] && !in_lu[pos]) o.uperm[lane] = (uint8_t)pos;
    }
}

void block(int ni, int nj, bool cyclic_ew, bool cyclic_ns, const uint8_t *mask, Block &B)
{
    const int H = W, LW = W + 1;
    const int nx = ni + 2, ny = nj + 2, ilo = 2, ihi = ni + 1, jlo = 2, jhi = nj + 1;      // 1-based, as in the kernels
    B.gx = (ni + W - 2) / (W - 1);
    B.gy = (nj + H - 2) / (H - 1);
    const int ntiles = B.gx * B.gy;
    B.cls.assign((size_t)ntiles * NPOS, 0);
    B.ice.assign((size_t)ntiles * NPOS, 0);
    B.uown.assign((size_t)ntiles * NPOS, 0);
    B.upub.assign((size_t)ntiles * NPOS, 0);
    B.tiles.resize((size_t)ntiles);
    // the interior cell a ghost cell mirrors, or -1
    auto ghost_src = [&](int pi, int pj, int &si, int &sj) -> bool {
        si = pi; sj = pj;
        if (pi < ilo || pi > ihi) {
            if (!cyclic_ew) return false;
            si = pi < ilo ? pi + ni : pi - ni;
        }
        if (pj < jlo || pj > jhi) {
            if (!cyclic_ns) return false;
            sj = pj < jlo ? pj + nj : pj - nj;
        }
        return si >= ilo && si <= ihi && sj >= jlo && sj <= jhi;
    };
    std::vector<uint8_t> pub((size_t)nx * ny, 0);      // per cell: polled by a tile that does not own it, or the source of a ghost image
    std::vector<uint8_t> ringli((size_t)(H + 1) * LW);
    // every ghost cell with a source is an image of it, polled or not
    for (int pj = 1; pj <= ny; ++pj)
        for (int pi = 1; pi <= nx; ++pi) {
            if (pi >= ilo && pi <= ihi && pj >= jlo && pj <= jhi) continue;
            int si, sj;
            if (ghost_src(pi, pj, si, sj)) pub[(size_t)(sj - 1) * nx + (si - 1)] = 1;
        }
    for (int pass = 0; pass < 2; ++pass)
        for (int by = 0; by < B.gy; ++by)
            for (int bx = 0; bx < B.gx; ++bx) {
                const int t = by * B.gx + bx;
                const int i0 = ilo + bx * (W - 1), j0 = jlo + by * (H - 1);
                if (pass == 1) {       // pub is complete: the tile's tables
                    uint8_t *ice = &B.ice[(size_t)t * NPOS], *uown = &B.uown[(size_t)t * NPOS], *upub = &B.upub[(size_t)t * NPOS];
                    for (int pos = 0; pos < NPOS; ++pos) {
                        const int tcol = pos % W, trow = pos / W, i = i0 + tcol, j = j0 + trow;
                        if (i > ihi + 1 || j > jhi + 1) continue;
                        const size_t cp = (size_t)(j - 1) * nx + (i - 1);
                        ice[pos] = (mask[cp] & 3u) != 0;
                        uown[pos] = tcol < W - 1 && trow < H - 1 && i <= ihi && j <= jhi;
                        upub[pos] = uown[pos] && pub[cp];
                    }
                    tile(&B.cls[(size_t)t * NPOS], ice, uown, upub, B.tiles[(size_t)t]);
                    continue;
                }
                std::fill(ringli.begin(), ringli.end(), 0);
                for (int trow = 0; trow < H; ++trow)
                    for (int tcol = 0; tcol < W; ++tcol) {
                        const int i = i0 + tcol, j = j0 + trow;
                        if (i > ihi + 1 || j > jhi + 1) continue;          // T-cell not computed
                        for (int q = 0; q < 4; ++q) {
                            const int di = -(q & 1), dj = -(q >> 1);
                            const int pc = tcol + di, pr = trow + dj, pi = i + di, pj = j + dj;
                            const bool interior = pi >= ilo && pi <= ihi && pj >= jlo && pj <= jhi;
                            if (interior && pc >= 0 && pc <= W - 2 && pr >= 0 && pr <= H - 2) continue;      // the tile's own
                            int si, sj;
                            if (!interior && !ghost_src(pi, pj, si, sj)) continue;      // nobody produces it
                            ringli[(size_t)(pr + 1) * LW + (pc + 1)] = 1;
                            if (interior) pub[(size_t)(pj - 1) * nx + (pi - 1)] = 1;
                            else pub[(size_t)(sj - 1) * nx + (si - 1)] = 1;
                        }
                    }
                for (int trow = 0; trow < H; ++trow)
                    for (int tcol = 0; tcol < W; ++tcol) {
                        const int i = i0 + tcol, j = j0 + trow;
                        const bool computed = i <= ihi + 1 && j <= jhi + 1;
                        const int li = (trow + 1) * LW + (tcol + 1);
                        const bool late = computed && (ringli[li] || ringli[li - 1] || ringli[li - LW] || ringli[li - LW - 1]);
                        B.cls[(size_t)t * NPOS + trow * W + tcol] = late ? 2 : computed ? 1 : 0;
                    }
            }
    B.ok = true;
    for (const Tile &tl : B.tiles) B.ok = B.ok && tl.ok;
}

}  // namespace rim_plan
