#include "cgrid_plan.h"
#include "evp_device.h"          // EVP_CGS_*: the bits of a zone / rest plan's cells

#include <algorithm>

namespace {
// The cell a position's value comes from: start at the nearest interior cell of the window's block and walk, x first, then
// y, one array cell at a time.  Stepping onto a ghost cell that mirrors an interior cell continues FROM that interior cell
// (through periodic boundaries and into other blocks); a ghost cell nothing is copied into (closed boundary, eliminated
// neighbour) is an array cell like any other and the walk goes on through it while it stays inside the block's array --
// so a position outside the domain names the ghost cell that IS the array neighbour of the cells next to it (a position
// reached through a periodic wrap used to name the block's own corner ghost cell instead: the same "outside", but not the
// cell the reference reads there, and its static arrays need not agree -- round 5, the on-chip resident C-grid kernel).
struct WindowWalk {
    const cice_evp_hip_dims &d;
    int nxb, nyb;
    long plane;
    std::vector<int> owner;
    WindowWalk(const cice_evp_hip_dims &d_, const HaloPlan &P) : d(d_), nxb(d_.nx_block), nyb(d_.ny_block), plane((long)d_.nx_block * d_.ny_block)
    {
        owner.assign((size_t)plane * d.nblocks, -1);
        for (size_t k = 0; k < P.local_dst.size(); ++k) owner[P.local_dst[k]] = P.local_src[k];
    }
    bool interior(int b, int i, int j) const { return i >= d.ilo[b] && i <= d.ihi[b] && j >= d.jlo[b] && j <= d.jhi[b]; }
    long walk(int b, int i, int j, int ti, int tj) const               // from interior (b, i, j) by (ti, tj) steps
    {
        bool stat = false;
        auto step = [&](int di, int dj) {
            const int ni = i + di, nj = j + dj;
            if (ni < 1 || ni > nxb || nj < 1 || nj > nyb) return;      // (beyond the array: stay -- two steps outside a closed boundary)
            i = ni; j = nj;
            if (interior(b, i, j)) { stat = false; return; }
            const long c = (long)b * plane + (long)(j - 1) * nxb + (i - 1);
            if (owner[c] >= 0) {
                const long o = owner[c];
                b = (int)(o / plane);
                j = (int)((o % plane) / nxb) + 1;
                i = (int)((o % plane) % nxb) + 1;
                stat = false;
            } else {
                stat = true;
            }
        };
        for (; ti != 0; ti -= (ti > 0 ? 1 : -1)) step(ti > 0 ? 1 : -1, 0);
        for (; tj != 0; tj -= (tj > 0 ? 1 : -1)) step(0, tj > 0 ? 1 : -1);
        const long c = (long)b * plane + (long)(j - 1) * nxb + (i - 1);
        return stat ? -1 - c : c;
    }
    long at(int b, int i, int j) const                                 // window position (i, j) in block b's index space
    {
        const int ic = std::min(std::max(i, d.ilo[b]), d.ihi[b]);
        const int jc = std::min(std::max(j, d.jlo[b]), d.jhi[b]);
        return walk(b, ic, jc, i - ic, j - jc);
    }
};
}   // namespace

void build_window_table(const cice_evp_hip_dims &d, const HaloPlan &P, int OX, int OY, int strip, std::vector<int32_t> &tiles,
                        std::vector<int32_t> &tab, int extra)
{
    const int nxb = d.nx_block, nyb = d.ny_block;
    const long plane = (long)nxb * nyb;
    const WindowWalk W(d, P);
    tiles.clear();
    tab.clear();
    strip = std::max(1, strip);
    for (int b = 0; b < d.nblocks; ++b)
        for (long is0 = d.ilo[b]; is0 <= d.ihi[b]; is0 += (long)strip * (OX - 3))
            for (int j0 = d.jlo[b]; j0 <= d.jhi[b]; j0 += OY - 3)
                for (long i0 = is0; i0 <= d.ihi[b] && i0 < is0 + (long)strip * (OX - 3); i0 += OX - 3) {
                    bool regular = true;
                    // (extra = 1: one more row and column of positions per window, same owned range -- the on-chip resident
                    // kernel's velocity tile, evp_cgrid_res.hip)
                    for (int ty = 0; ty < OY + extra; ++ty)
                        for (int tx = 0; tx < OX + extra; ++tx) {
                            const int i = (int)i0 - 2 + tx, j = j0 - 2 + ty;
                            const long r = W.at(b, i, j);
                            tab.push_back((int32_t)r);
                            regular = regular && i >= 1 && i <= nxb && j >= 1 && j <= nyb &&
                                      r == (long)b * plane + (long)(j - 1) * nxb + (i - 1);
                        }
                    tiles.push_back(b);
                    tiles.push_back((int32_t)i0);
                    tiles.push_back(j0);
                    tiles.push_back(regular ? 1 : 0);
                }
}

void strip_zones(const cice_evp_hip_dims &d, const std::vector<int32_t> &tiles, int ex, int ey, const int *img_slot, std::vector<StripZone> &zones,
                 int min_cols)
{
    const int nt = (int)(tiles.size() / 4), sx = ex - 3, sy = ey - 3;
    zones.clear();
    for (int b = 0; b < d.nblocks; ++b) {
        int i0 = 1 << 30, i1 = -1, j0 = 1 << 30, j1 = -1, cnt = 0;
        for (int w = 0; w < nt; ++w)
            if (tiles[4 * w] == b && tiles[4 * w + 3]) {
                i0 = std::min(i0, tiles[4 * w + 1]); i1 = std::max(i1, tiles[4 * w + 1]);
                j0 = std::min(j0, tiles[4 * w + 2]); j1 = std::max(j1, tiles[4 * w + 2]);
                ++cnt;
            }
        if (!cnt || (i1 - i0) % sx || (j1 - j0) % sy) continue;
        if (cnt != ((i1 - i0) / sx + 1) * ((j1 - j0) / sy + 1)) continue;       // (not a rectangle: cg_one keeps the block)
        // (the kernel's loads inside the array: a rectangle whose last owned row is jhi - 1 would prefetch row ny_block + 1)
        while (j1 >= j0 && i1 + sx - i0 >= min_cols) {
            StripRange r{1 << 30, -(1 << 30), 1 << 30, -(1 << 30)};
            std::vector<int32_t> it;
            const std::vector<StripZone> one{StripZone{b, i0, i1, j0, j1}};
            for (int lo0 = 2; lo0 <= 3; ++lo0) {
                strip_items(one, ex, ey, lo0, 1, 1, j1 - j0 + sy, it);
                for (size_t k = 0; k < it.size(); k += 6) {
                    const StripRange f = strip_footprint(&it[k], lo0 == 3);
                    r = StripRange{std::min(r.i0, f.i0), std::max(r.i1, f.i1), std::min(r.j0, f.j0), std::max(r.j1, f.j1)};
                }
            }
            if (r.j1 > d.ny_block) j1 -= sy;
            else if (r.j0 < 1) j0 += sy;
            else if (r.i1 > d.nx_block) i1 -= sx;
            else if (r.i0 < 1) i0 += sx;
            else break;
        }
        if (j1 < j0) continue;
        if (i1 + sx - i0 < min_cols) continue;                                    // (narrower than a strip)
        // (cells with ghost images -- the block's outermost interior cells -- never lie inside: the marched kernel has no pushes)
        bool images = false;
        for (int j = j0; j <= j1 + sy - 1 && !images && img_slot; ++j)
            for (int i = i0; i <= i1 + sx - 1 && !images; ++i)
                images = img_slot[(size_t)b * d.nx_block * d.ny_block + (size_t)(j - 1) * d.nx_block + (i - 1)] >= 0;
        if (images) continue;
        zones.push_back(StripZone{b, i0, i1, j0, j1});
    }
}

int strip_items(const std::vector<StripZone> &zones, int ex, int ey, int lo0, long slots, int seg_min, int seg, std::vector<int32_t> &items)
{
    const int sx = ex - 3, sy = ey - 3, sown = 62 - lo0;
    items.clear();
    long nstrips = 0, maxrows = 0;
    for (const StripZone &z : zones) { nstrips += (z.i1 - z.i0 + sx + sown - 1) / sown; maxrows = std::max<long>(maxrows, z.j1 - z.j0 + sy); }
    if (seg <= 0) {
        const long nseg_fit = std::max<long>(1, slots / std::max<long>(1, nstrips));
        seg = (int)std::max<long>(seg_min, (maxrows + nseg_fit - 1) / nseg_fit);
    }
    for (const StripZone &z : zones) {
        const int rows = z.j1 - z.j0 + sy, nseg = (rows + seg - 1) / seg;
        const int ilast = z.i1 + sx - 1;                       // last owned column of the rectangle
        for (int k = 0; k < nseg; ++k) {
            // (equal segments: rows / nseg, the remainder one row each to the first ones)
            const int ja = z.j0 + (int)((long)rows * k / nseg), jb = z.j0 + (int)((long)rows * (k + 1) / nseg) - 1;
            for (int i0 = z.i0; i0 <= ilast; i0 += sown) {
                // column of lane 2: the strip's first owned column on lane lo0, or further west if lane 61 would pass the rectangle
                const int c = std::min(i0 - (lo0 - 2), std::max(z.i0 - (lo0 - 2), ilast - 59));
                const int lo = 2 + (i0 - c), hi = std::min(61, 2 + (ilast - c));
                items.push_back(z.b); items.push_back(c); items.push_back(ja); items.push_back(jb);
                items.push_back(lo); items.push_back(hi);
            }
        }
    }
    return seg;
}

bool strip_len_range(const StripZone &z, int ex, int ey, int nx_block, int ny_block, StripRange &r)
{
    // (strip_items with lo0 = 3: the first strip's lane 2 on column i0 - 1, the last strip's lane 61 on the last owned column)
    const int sx = ex - 3, sy = ey - 3;
    r = StripRange{z.i0 - 3, z.i1 + sx - 1 + 2, z.j0 - 2, z.j1 + sy - 1 + 2};
    // (dxE reads HTN at i + 1 and j - 1, dyN HTE at i - 1 and j + 1, dxT HTN at j - 1, dyT HTE at i - 1 ...)
    return r.i0 >= 2 && r.i1 <= nx_block - 1 && r.j0 >= 2 && r.j1 <= ny_block - 1;
}

void strip_windows(const std::vector<StripZone> &zones, const std::vector<int32_t> &tiles, std::vector<uint8_t> &in_zone)
{
    const int nt = (int)(tiles.size() / 4);
    in_zone.assign((size_t)nt, 0);
    for (const StripZone &z : zones)
        for (int w = 0; w < nt; ++w)
            if (tiles[4 * w] == z.b && tiles[4 * w + 3] && tiles[4 * w + 1] >= z.i0 && tiles[4 * w + 1] <= z.i1 &&
                tiles[4 * w + 2] >= z.j0 && tiles[4 * w + 2] <= z.j1)
                in_zone[(size_t)w] = 1;
}

void plan_strip_zones(const cice_evp_hip_dims &d, const HaloPlan &P, int ex, int ey, int min_cols, int last_image_row, std::vector<int32_t> &tiles,
                      std::vector<StripZone> &zones)
{
    std::vector<int32_t> tab;
    build_window_table(d, P, ex, ey, 1 << 20, tiles, tab);
    // ghost images: the sources of the rank's own ghost copies (-1: a ghost cell filled with 0, no source)
    const long plane = (long)d.nx_block * d.ny_block;
    std::vector<int> img((size_t)plane * d.nblocks, -1);
    for (size_t k = 0; k < P.local_src.size(); ++k) {
        if (P.local_src[k] < 0) continue;
        if (last_image_row != STRIP_EVERY_IMAGE) {
            const int db = (int)(P.local_dst[k] / plane), dj = (int)((P.local_dst[k] % plane) / d.nx_block) + 1;
            if (d.jglob0[db] + (dj - d.jlo[db]) > last_image_row) continue;
        }
        img[(size_t)P.local_src[k]] = 0;
    }
    strip_zones(d, tiles, ex, ey, img.data(), zones, min_cols);
}

namespace {
// ---- a rank's interior cells split between cg_strip (the zone) and list-driven kernels (the rest): what build_cg_frame and
// build_cg_march_fold share (cgrid_plan.h) ----
// One read of the list-driven chain: a cell on which level `reader` runs reads `what` -- the text of the check that fails -- at these
// offsets from itself, and level `producer` makes it.  A plan lists its reads from the last level of a subcycle back to the first, every
// level complete before the reads OF it come; marking (dilate) and checking (check_cell) walk the same table.
struct CgRead {
    int reader, producer, n;
    int at[8][2];
    const char *what;
};
// the words in which the two plans' error texts differ
struct CgSplitWords {
    const char *plan, *sum, *ghost, *own, *t_loads;
    bool near;          // a read nobody produces is reported at the reading cell ("..., near"), not at the cell read
};
struct CgSplit {
    const cice_evp_hip_dims &d;
    CgSplitPlan &F;
    std::string &why;
    const CgSplitWords &words;
    const std::vector<CgRead> &reads;
    const int nxb, nyb;
    const long plane;
    int own_levels = 0, not_t = 0;       // the levels a rest cell runs itself; everything that may not run on a ghost cell
    long n_interior = 0;
    CgSplit(const cice_evp_hip_dims &d_, CgSplitPlan &F_, std::string &why_, const CgSplitWords &w, const std::vector<CgRead> &r)
        : d(d_), F(F_), why(why_), words(w), reads(r), nxb(d_.nx_block), nyb(d_.ny_block), plane((long)d_.nx_block * d_.ny_block)
    {
        for (const CgRead &q : reads) own_levels |= q.reader | q.producer;
        not_t = own_levels & ~EVP_CGS_T;
        own_levels &= ~EVP_CGS_REST;
    }
    size_t off(int b, int i, int j) const { return (size_t)b * plane + (size_t)(j - 1) * nxb + (size_t)(i - 1); }
    bool inside(int i, int j) const { return i >= 1 && i <= nxb && j >= 1 && j <= nyb; }
    bool interior(int b, int i, int j) const { return i >= d.ilo[b] && i <= d.ihi[b] && j >= d.jlo[b] && j <= d.jhi[b]; }
    void cell_of(size_t c, int &b, int &i, int &j) const
    {
        b = (int)(c / (size_t)plane);
        j = (int)((c % (size_t)plane) / nxb) + 1;
        i = (int)((c % (size_t)plane) % nxb) + 1;
    }
    int bad(const char *what, int b, int i, int j) const
    {
        char buf[200];
        std::snprintf(buf, sizeof buf, "%s: %s at block %d cell (%d, %d)", words.plan, what, b, i, j);
        why = buf;
        return -1;
    }
    // ownership: the items' cells are the zone, everything else of the interior the rest
    int own(const std::vector<int32_t> &items)
    {
        F.cells.assign((size_t)plane * d.nblocks, 0);
        for (size_t k = 0; k + 5 < items.size(); k += 6) {
            const int b = items[k], c = items[k + 1], ja = items[k + 2], jb = items[k + 3], lo = items[k + 4], hi = items[k + 5];
            if (b < 0 || b >= d.nblocks) return bad("an item of a block that is not here", b, c, ja);
            for (int j = ja; j <= jb; ++j)
                for (int i = c - 2 + lo; i <= c - 2 + hi; ++i) {
                    if (!interior(b, i, j)) return bad("a marched cell outside the interior", b, i, j);
                    uint8_t &f = F.cells[off(b, i, j)];
                    if (f & EVP_CGS_ZONE) return bad("a cell two items own", b, i, j);
                    f |= EVP_CGS_ZONE;
                    ++F.zone_cells;
                }
        }
        n_interior = 0;
        for (int b = 0; b < d.nblocks; ++b)
            for (int j = d.jlo[b]; j <= d.jhi[b]; ++j)
                for (int i = d.ilo[b]; i <= d.ihi[b]; ++i) {
                    ++n_interior;
                    uint8_t &f = F.cells[off(b, i, j)];
                    if (!(f & EVP_CGS_ZONE)) {
                        f |= EVP_CGS_REST;
                        ++F.rest_cells;
                    }
                }
        return 0;
    }
    // the levels, each dilated by what the next one reads of it
    int dilate()
    {
        // the reference's T list: stress12T of the ghost row and column i = ihi + 1, j = jhi + 1 -- level T there, and nothing else
        for (int b = 0; b < d.nblocks; ++b)
            for (int j = d.jlo[b]; j <= d.jhi[b] + 1; ++j)
                for (int i = d.ilo[b]; i <= d.ihi[b] + 1; ++i) {
                    if (!inside(i, j)) return bad("the extra T row / column outside the array", b, i, j);
                    if (!interior(b, i, j)) F.cells[off(b, i, j)] |= EVP_CGS_T;
                }
        for (const CgRead &r : reads)
            for (int b = 0; b < d.nblocks; ++b)
                for (int j = d.jlo[b]; j <= d.jhi[b] + 1; ++j) {
                    const uint8_t *row = &F.cells[off(b, 1, j)] - 1;
                    for (int i = d.ilo[b]; i <= d.ihi[b] + 1; ++i)
                        if (row[i] & r.reader)
                            for (int q = 0; q < r.n; ++q)
                                if (interior(b, i + r.at[q][0], j + r.at[q][1])) F.cells[off(b, i + r.at[q][0], j + r.at[q][1])] |= (uint8_t)r.producer;
                }
        return 0;
    }
    int check_sum() const { return F.zone_cells + F.rest_cells == n_interior ? 0 : bad(words.sum, 0, 0, 0); }
    // the invariants of one array cell
    int check_cell(int b, int i, int j) const
    {
        const uint8_t f = F.cells[off(b, i, j)];
        const bool in = interior(b, i, j);
        if ((f & EVP_CGS_ZONE) && (f & EVP_CGS_REST)) return bad("a cell in both sets", b, i, j);
        if (in != ((f & (EVP_CGS_ZONE | EVP_CGS_REST)) != 0)) return bad("a cell of neither set, or a ghost cell of one", b, i, j);
        if (!(f & (not_t | EVP_CGS_T))) return 0;          // (no level runs here)
        if ((f & not_t) && !in) return bad(words.ghost, b, i, j);
        if ((f & EVP_CGS_REST) && (f & own_levels) != own_levels) return bad(words.own, b, i, j);
        for (const CgRead &r : reads) {
            if (!(f & r.reader)) continue;
            if (r.reader == EVP_CGS_T)           // (the one level that runs on ghost cells)
                for (int q = 0; q < r.n; ++q)
                    if (!inside(i + r.at[q][0], j + r.at[q][1])) return bad(words.t_loads, b, i, j);
            for (int q = 0; q < r.n; ++q) {
                const int ri = i + r.at[q][0], rj = j + r.at[q][1];
                if (interior(b, ri, rj) && !(F.cells[off(b, ri, rj)] & r.producer)) return words.near ? bad(r.what, b, i, j) : bad(r.what, b, ri, rj);
            }
        }
        // (every level but T: the velocities, lengths and masks one cell around the cell)
        if ((f & not_t) && !(inside(i - 1, j - 1) && inside(i + 1, j + 1))) return bad("a stencil outside the array", b, i, j);
        return 0;
    }
    // wg[k]: the workgroups of 64 x 4 cells that hold a cell of level bits[k]
    void workgroups(std::initializer_list<int> bits)
    {
        const int gx = (nxb + 63) / 64, gy = (nyb + 3) / 4;
        int k = 0;
        for (int bit : bits) {
            std::vector<uint8_t> on((size_t)gx * gy * d.nblocks, 0);
            for (int b = 0; b < d.nblocks; ++b)
                for (int j = 1; j <= nyb; ++j)
                    for (int i = 1; i <= nxb; ++i)
                        if (F.cells[off(b, i, j)] & bit) on[((size_t)b * gy + (size_t)(j - 1) / 4) * gx + (size_t)(i - 1) / 64] = 1;
            for (size_t w = 0; w < on.size(); ++w)
                if (on[w]) F.wg[k].push_back((int32_t)w);
            ++k;
        }
    }
};
}   // namespace

int build_cg_frame(const cice_evp_hip_dims &d, const HaloPlan &P, const std::vector<int32_t> &items, CgFramePlan &F, std::string &why)
{
    F = CgFramePlan();
    why.clear();
    if (P.peers.empty() && P.cg_peers.empty()) {
        why = "no neighbour on another rank";
        return 0;
    }
    // level C reads etax2T around its three corners (the new stresspT, stressmT of the east and north neighbour are among those T cells) and
    // shearU at its own, south and west corner; level T reads shearU at its four corners
    static const std::vector<CgRead> reads = {
        {EVP_CGS_REST, EVP_CGS_T, 8, {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {0, -1}, {1, -1}, {-1, 0}, {-1, 1}}, "etax2T read where level T does not run"},
        {EVP_CGS_REST, EVP_CGS_S, 3, {{0, 0}, {0, -1}, {-1, 0}}, "shearU read where level S does not run"},
        {EVP_CGS_T, EVP_CGS_S, 4, {{0, 0}, {0, -1}, {-1, -1}, {-1, 0}}, "shearU read where level S does not run"},
    };
    static const CgSplitWords words = {"frame plan", "zone and frame do not add up to the interior", "level S or C on a ghost cell",
                                       "a frame cell without its own levels", "level T loads outside the array", false};
    CgSplit X(d, F, why, words, reads);
    if (X.own(items) || X.dilate() || X.check_sum()) return -1;
    // what leaves the rank, or has an image on it, is the frame's: the marched kernel has no pushes and runs beside the exchange
    auto must_be_frame = [&](int32_t c, const char *what) {
        if (c < 0 || (size_t)c >= F.cells.size()) return 0;          // (a staging slot behind the array: no cell)
        if (F.cells[(size_t)c] & EVP_CGS_REST) return 0;
        int b, i, j;
        X.cell_of((size_t)c, b, i, j);
        return X.bad(what, b, i, j);
    };
    for (const std::vector<HaloPeer> *pp : {&P.peers, &P.cg_peers})
        for (const HaloPeer &p : *pp)
            for (int32_t c : p.send_src)
                if (must_be_frame(c, "a cell another rank receives is not a frame cell")) return -1;
    for (size_t k = 0; k < P.local_src.size(); ++k)
        if (P.local_src[k] >= 0 && must_be_frame(P.local_src[k], "a cell with a ghost image is not a frame cell")) return -1;
    for (int b = 0; b < d.nblocks; ++b)
        for (int j = 1; j <= d.ny_block; ++j)
            for (int i = 1; i <= d.nx_block; ++i)
                if (X.check_cell(b, i, j)) return -1;
    X.workgroups({EVP_CGS_S, EVP_CGS_T, EVP_CGS_REST});
    return 1;
}

int build_cg_march_fold(const cice_evp_hip_dims &d, const HaloPlan &P, int ex, int ey, long slots, int seg_min, int seg, int want_len,
                        const CgGeoCheck *geo, CgMarchFoldPlan &F, std::string &why, bool allow_ranks)
{
    F = CgMarchFoldPlan();
    why.clear();
    const bool tf = d.ns_boundary_type == CICE_EVP_BND_TRIPOLET;
    const bool folded = d.ns_boundary_type == CICE_EVP_BND_TRIPOLE || tf;
    const bool ranks = !P.peers.empty() || !P.cg_peers.empty();
    // (no fold, several ranks: the same plan with the frame as the whole REST -- no fold cells, no rows cut from the top)
    if (!folded && !(ranks && allow_ranks)) {
        why = "no tripole fold (the one-launch schedule marches such a grid)";
        return 0;
    }
    if (ranks && !allow_ranks) {
        why = "several ranks, or the fold rows not on this rank";
        return 0;
    }
    if (folded && !ranks && (P.cg_split || P.fold_rows != 1)) {
        why = "several ranks, or the fold rows not on this rank";
        return 0;
    }
    if (folded && P.fold_rows == 2 && !P.cg_split) {
        why = "the fold rows shared with other ranks without the C grid's fold exchange";
        return 0;
    }
    if (d.nx_block < 3 || d.ny_block < 3 || (folded && d.nx_global % 2)) {
        why = "a block too small";
        return 0;
    }
    // the five phases, from the momentum step back (offsets from the evaluating cell); phase 4, the averages, runs AFTER the two sets have
    // met again: on the rest cells and on what phase 0 of the next subcycle reads
    static const std::vector<CgRead> reads = {
        {EVP_CGS_REST, EVP_CGS_U, 3, {{0, 0}, {0, -1}, {-1, 0}}, "stress12U read where phase 2 does not run, near"},
        {EVP_CGS_REST, EVP_CGS_T, 3, {{0, 0}, {1, 0}, {0, 1}}, "stresspT read where phase 1 does not run, near"},          // and stressmT
        {EVP_CGS_U, EVP_CGS_T, 4, {{0, 0}, {1, 0}, {0, 1}, {1, 1}}, "etax2T / shearU read where it is not produced, near"},
        {EVP_CGS_U, EVP_CGS_S, 1, {{0, 0}}, "etax2T / shearU read where it is not produced, near"},
        {EVP_CGS_T, EVP_CGS_S, 4, {{0, 0}, {0, -1}, {-1, -1}, {-1, 0}}, "shearU read where phase 0 does not run, near"},
        {EVP_CGS_REST, EVP_CGS_AVG, 1, {{0, 0}}, "a REST cell without its own levels"},
        // uvelN (own, east), vvelE (own, north), uvelU, vvelU (own)
        {EVP_CGS_S, EVP_CGS_AVG, 3, {{0, 0}, {1, 0}, {0, 1}}, "an average read where phase 4 does not run, near"},
    };
    static const CgSplitWords words = {"fold-band plan", "zone and rest do not add up to the interior", "a phase other than stressC_T on a ghost cell",
                                       "a REST cell without its own levels", "phase 1 loads outside the array", true};
    // (without a fold the same plan under its own name: a failure at set_geometry must not send its reader to a fold)
    static const CgSplitWords words_no_fold = {"five-phase frame plan", "zone and rest do not add up to the interior", "a phase other than stressC_T on a ghost cell",
                                               "a REST cell without its own levels", "phase 1 loads outside the array", true};
    CgSplit X(d, F, why, folded ? words : words_no_fold, reads);
    const int nxb = d.nx_block, nyb = d.ny_block, NY = d.ny_global, sy = ey - 3;
    const size_t ncell = (size_t)nxb * nyb * d.nblocks;
    auto grow = [&](int b, int j) { return d.jglob0[b] + (j - d.jlo[b]); };          // global row of local row j
    // on the fold or beyond it, by field location (0 centre, 1 NE corner, 2 E face, 3 N face) and global row
    auto at_fold = [&](int loc, int jg) { return folded && (jg > NY || (jg == NY && (tf || loc == 1 || loc == 3))); };
    // ---- the fold step's cells: destinations and sources of every location ----
    std::vector<uint8_t> foldcell(ncell, 0);
    // (the lists the host runs: the C grid's own where the fold rows have several owners -- operands >= ncell are staging slots the
    // exchange fills --, build_fold_list's where they are all here, none on a rank without them)
    FoldList L[4];
    for (int loc = 0; loc < 4; ++loc) {
        if (!folded) break;
        if (P.cg_split) L[loc] = P.cg_fold[loc];
        else if (P.fold_rows == 1) build_fold_list(d, loc, L[loc]);
        for (size_t k = 0; k < L[loc].dst.size(); ++k)
            for (int32_t c : {L[loc].dst[k], L[loc].a[k], L[loc].b[k]}) {
                if (c >= 0 && (size_t)c < ncell) foldcell[(size_t)c] = 1;
                else if (c >= 0 && (size_t)c >= ncell + (size_t)P.cg_tail) return X.bad("a fold-list operand behind the staging slots", 0, 0, 0);
            }
    }
    // ---- the FRAME: what leaves the rank in an in-loop exchange -- ghost cells of the peers and, in the C grid's lists, the raw fold
    // sources for their staging slots -- and what has a ghost image here.  The marched kernel has no pushes and runs beside the
    // exchanges: none of these may be a zone cell (the fold sources come off a rectangle's top with the fold step's own cells) ----
    std::vector<uint8_t> frame(ncell, 0);
    for (const std::vector<HaloPeer> *pp : {&P.peers, &P.cg_peers})
        for (const HaloPeer &p : *pp)
            for (int32_t c : p.send_src)
                if (c >= 0 && (size_t)c < ncell && !frame[(size_t)c]) {
                    frame[(size_t)c] = 1;
                    foldcell[(size_t)c] = 1;
                    F.sent.push_back(c);
                }
    std::sort(F.sent.begin(), F.sent.end());
    for (int32_t c : P.local_src)
        if (c >= 0 && (size_t)c < ncell) frame[(size_t)c] = 1;
    // ---- the rectangles, cut from the top until the fold rule holds ----
    // (ghost cells the fold step fills -- the row beyond the fold, on a T-fold the top physical row too -- are no images: their sources
    // are fold cells, which come off the rectangle's top below instead of costing a block its rectangle.  A rectangle narrower than a
    // strip is one item per segment with fewer owned lanes: tx3's 100 columns hold two regular window columns, 58 cells; the footprint
    // check below keeps its lanes inside the array)
    std::vector<int32_t> tiles;
    std::vector<StripZone> zones0, zones;
    plan_strip_zones(d, P, ex, ey, ex - 3, folded ? NY - (tf ? 1 : 0) : STRIP_EVERY_IMAGE, tiles, zones0);
    bool len_all = want_len != 0;
    for (StripZone z : zones0) {
        auto rule_holds = [&]() {
            // (the items of a rectangle share its top row: the segment that ends there decides)
            const int jb = z.j1 + sy - 1;
            for (int loc = 0; loc < 4; ++loc)
                if (at_fold(loc, grow(z.b, jb + strip_form_top(loc)))) return false;
            std::vector<int32_t> it;
            const std::vector<StripZone> one{z};
            for (int lo0 = 2; lo0 <= 3; ++lo0) {
                strip_items(one, ex, ey, lo0, 1, 1, z.j1 - z.j0 + sy, it);
                for (size_t k = 0; k < it.size(); k += 6) {
                    const StripRange f = strip_footprint(&it[k], lo0 == 3);
                    if (f.i0 < 1 || f.i1 > nxb || f.j0 < 1 || f.j1 > nyb || (folded && grow(z.b, f.j1) > NY + 1)) return false;
                }
            }
            for (int j = z.j0; j <= jb; ++j)
                for (int i = z.i0; i <= z.i1 + ex - 3 - 1; ++i)
                    if (foldcell[X.off(z.b, i, j)]) return false;
            return true;
        };
        int g = 0;
        while (z.j1 >= z.j0) {
            if (rule_holds() && (g = geo ? (*geo)(z) : 3) != 0) break;
            z.j1 -= sy;
        }
        if (z.j1 < z.j0) continue;
        len_all = len_all && g == 3;
        zones.push_back(z);
    }
    if (zones.empty()) {
        why = folded ? "no rectangle for the marched kernel is left under the fold band" : "no rectangle for the marched kernel on this rank";
        return 0;
    }
    F.zones = zones;
    F.lengths = len_all ? 1 : 0;
    long zcells = 0;
    for (const StripZone &z : zones) zcells += (long)(z.i1 - z.i0 + ex - 3) * (z.j1 - z.j0 + sy);
    F.seg = strip_items(zones, ex, ey, F.lengths ? 3 : 2, slots, seg_min > 0 ? seg_min : (zcells >= 1000000 ? 16 : 8), seg, F.items);
    for (int b = 0; b < d.nblocks; ++b) {
        if (!folded || grow(b, d.jhi[b]) != NY) continue;
        int top = d.jlo[b] - 1;
        for (const StripZone &z : zones)
            if (z.b == b) top = std::max(top, z.j1 + sy - 1);
        F.band_rows = std::max(F.band_rows, NY - grow(b, top));          // (a block at the fold without a rectangle: all its rows)
    }
    // ---- the two sets, the fold row, the phases ----
    if (X.own(F.items)) return -1;
    for (int b = 0; b < d.nblocks; ++b)
        if (folded && grow(b, d.jhi[b]) == NY)
            for (int i = d.ilo[b]; i <= d.ihi[b]; ++i) F.cells[X.off(b, i, d.jhi[b])] |= EVP_CGS_FOLDROW;
    if (X.dilate() || X.check_sum()) return -1;
    // ---- the invariants ----
    static const int level_of_loc[4] = {EVP_CGS_T, EVP_CGS_U, EVP_CGS_REST, EVP_CGS_REST};   // who produces a field of this location (phase 4's
    for (int loc = 0; loc < 4; ++loc)                                                         // fields: EVP_CGS_AVG, checked with it)
        for (size_t k = 0; k < L[loc].dst.size(); ++k)
            for (int32_t c : {L[loc].dst[k], L[loc].a[k], L[loc].b[k]}) {
                if (c < 0 || (size_t)c >= ncell) continue;
                int b, i, j;
                X.cell_of((size_t)c, b, i, j);
                if (!X.interior(b, i, j)) continue;
                const uint8_t f = F.cells[(size_t)c];
                if (!(f & EVP_CGS_REST)) return X.bad("a cell of the fold step is not a REST cell", b, i, j);
                if (!(f & level_of_loc[loc]) || !(f & EVP_CGS_AVG) || !(f & EVP_CGS_S)) return X.bad("a cell of the fold step is not evaluated at its level", b, i, j);
            }
    // (every sent cell runs the level that produces the field it is sent for: a REST cell runs them all; so does a cell with an image)
    constexpr int every_level = EVP_CGS_REST | EVP_CGS_S | EVP_CGS_T | EVP_CGS_U | EVP_CGS_AVG;
    for (size_t c = 0; c < ncell; ++c) {
        if (!frame[c]) continue;
        int b, i, j;
        X.cell_of(c, b, i, j);
        if (!X.interior(b, i, j)) return X.bad("a sent cell or the source of a ghost image is no interior cell", b, i, j);
        if ((F.cells[c] & every_level) != every_level)
            return X.bad("a cell another rank receives, or one with a ghost image, is not a REST cell evaluated at every level", b, i, j);
        ++F.frame_cells;
    }
    for (int b = 0; b < d.nblocks; ++b)
        for (int j = 1; j <= nyb; ++j)
            for (int i = 1; i <= nxb; ++i) {
                if (X.check_cell(b, i, j)) return -1;
                // (no item forms anything on the fold or beyond it)
                if (F.cells[X.off(b, i, j)] & EVP_CGS_ZONE)
                    for (int loc = 0; loc < 4; ++loc)
                        if (at_fold(loc, grow(b, j + strip_form_top(loc)))) return X.bad("the marched kernel forms a value on the fold above", b, i, j);
            }
    X.workgroups({EVP_CGS_S, EVP_CGS_T, EVP_CGS_U, EVP_CGS_REST, EVP_CGS_AVG});
    return 1;
}

int cgres_dependencies(const cice_evp_hip_dims &d, bool tripole, const std::vector<int32_t> &tiles, const std::vector<int32_t> &tab,
                       std::vector<uint8_t> *pub, int *n_edges, int *n_oneway)
{
    constexpr int RX = 16, RY = 16, LW = RX + 1, NPOS = LW * (RY + 1);
    const int nt = (int)(tiles.size() / 4);
    const size_t ncell = (size_t)d.nblocks * d.nx_block * d.ny_block;
    auto jmax_of = [&](int w) { return tripole ? (int)(tiles[4 * w + 3] >> 16) : (int)d.jhi[tiles[4 * w]]; };
    auto foldwin = [&](int w) { return tripole && (tiles[4 * w + 3] & 1); };
    auto mine = [&](int w, int ex, int ey) {
        const int b = tiles[4 * w], i0 = tiles[4 * w + 1], j0 = tiles[4 * w + 2];
        return ex >= 2 && ex <= RX - 2 && ey >= 2 && ey <= RY - 2 && i0 - 2 + ex <= d.ihi[b] && j0 - 2 + ey <= jmax_of(w);
    };
    std::vector<int32_t> owner(ncell, -1);
    for (int w = 0; w < nt; ++w)
        for (int e = 0; e < NPOS; ++e)
            if (mine(w, e % LW, e / LW)) {
                const int sc = tab[(size_t)w * NPOS + e];
                if (sc >= 0 && (size_t)sc < ncell) owner[(size_t)sc] = w;
            }
    if (pub) pub->assign(ncell, 0);
    std::vector<std::pair<int, int>> edges;
    for (int w = 0; w < nt; ++w) {
        const int b = tiles[4 * w], i0 = tiles[4 * w + 1], j0 = tiles[4 * w + 2];
        const int last_ex = std::min(RX - 2, 2 + d.ihi[b] - i0), last_ey = std::min(RY - 2, 2 + jmax_of(w) - j0);
        for (int e = 0; e < NPOS - 1; ++e) {              // ((RX, RY), the one entry no level reads, is left out)
            const int ex = e % LW, ey = e / LW;
            const int sc = tab[(size_t)w * NPOS + e];
            if (mine(w, ex, ey) || sc < 0 || !cgres_in_reach(ex, ey, last_ex, last_ey, foldwin(w))) continue;
            if (pub) (*pub)[(size_t)sc] = 1;
            const int p = owner[(size_t)sc];
            if (p >= 0 && p != w) edges.emplace_back(w, p);
        }
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    if (n_edges) *n_edges = (int)edges.size();
    // reads[w]: the windows w reads (edges is sorted by reader)
    std::vector<int> first((size_t)nt + 1, 0);
    for (const auto &e : edges) ++first[(size_t)e.first + 1];
    for (int w = 0; w < nt; ++w) first[(size_t)w + 1] += first[(size_t)w];
    int oneway = 0, unsafe = 0;
    std::vector<int> seen((size_t)nt, -1), frontier, next;
    int stamp = 0;
    for (const auto &e : edges) {
        if (std::binary_search(edges.begin(), edges.end(), std::make_pair(e.second, e.first))) continue;
        ++oneway;
        // w = e.first reads p = e.second and p does not read w: is there a chain p reads ... reads w of at most CGRES_SLOTS - 1?
        const int w = e.first, p = e.second;
        ++stamp;
        frontier.assign(1, p);
        seen[(size_t)p] = stamp;
        bool found = false;
        for (int len = 1; len <= CGRES_SLOTS - 1 && !found && !frontier.empty(); ++len) {
            next.clear();
            for (int x : frontier)
                for (int k = first[(size_t)x]; k < first[(size_t)x + 1] && !found; ++k) {
                    const int y = edges[(size_t)k].second;
                    if (y == w) found = true;
                    else if (seen[(size_t)y] != stamp) { seen[(size_t)y] = stamp; next.push_back(y); }
                }
            frontier.swap(next);
        }
        if (!found) ++unsafe;
    }
    if (n_oneway) *n_oneway = oneway;
    return unsafe;
}

// Windows of the on-chip resident C-grid kernel on a tripole (u-fold) grid (evp_cgrid_res.hip, template variant FOLD).  17 x 17
// positions per window, 13 x 13 owned as in build_window_table(..., extra = 1), except:
//  * the top window row of a block that touches the fold owns the block's last (up to) 11 rows, so that the fold row NY sits
//    at tile row tf <= 12 and three more tile rows remain; the window rows below it stop where it starts;
//  * tile rows tf+1 .. tf+3 of those windows hold a MIRRORED mini-tile in SOURCE orientation: global rows NY-2, NY-1, NY, tile
//    column tx <-> global column G0' + tx with G0' = NX - G0 - 15, G0 + tx = the global column of normal tile column tx.  A
//    normal fold-row position tx then faces the E-face / corner-type source at mirrored column 15 - tx and the centre / N-face
//    type source at 16 - tx (ice_boundary.F90:1626-1722: NX - ig for E faces and NE corners, NX - ig + 1 for centres and N
//    faces);
//  * tile rows above the mini-tile are unused (marked static, naming the window's first cell).
// tiles: (block, i0, j0, flags) with flags bit 0 = fold window, bits 8-15 = tf, bits 16-31 = last owned row (block index
// space); tiles2: (G0, NX, 0, 0).  Returns false (and says why) when a mirrored cell is not an interior cell of a block on
// this rank -- the resident kernel then is not used.
bool build_fold_window_table(const cice_evp_hip_dims &d, const HaloPlan &P, std::vector<int32_t> &tiles, std::vector<int32_t> &tiles2,
                             std::vector<int32_t> &tab, std::string &why)
{
    const int X = 16, OWN = 13, FOLDOWN = 11;
    const int nxb = d.nx_block;
    const long plane = (long)nxb * d.ny_block;
    const int NX = d.nx_global, NY = d.ny_global;
    const WindowWalk W(d, P);
    tiles.clear(); tiles2.clear(); tab.clear();
    std::vector<int32_t> cell((size_t)NX * NY, -1);                    // global (ig, jg) -> local interior cell
    for (int b = 0; b < d.nblocks; ++b)
        for (int j = d.jlo[b]; j <= d.jhi[b]; ++j)
            for (int i = d.ilo[b]; i <= d.ihi[b]; ++i) {
                const int ig = d.iglob0[b] + (i - d.ilo[b]), jg = d.jglob0[b] + (j - d.jlo[b]);
                if (ig >= 1 && ig <= NX && jg >= 1 && jg <= NY) cell[(size_t)(jg - 1) * NX + (ig - 1)] = (int32_t)(b * plane + (long)(j - 1) * nxb + (i - 1));
            }
    auto wrap = [&](long ig) { ig = (ig - 1) % NX; if (ig < 0) ig += NX; return (int)ig + 1; };
    for (int b = 0; b < d.nblocks; ++b) {
        const bool top = d.jglob0[b] + (d.jhi[b] - d.jlo[b]) == NY;
        const int jtop = top ? std::max(d.jlo[b], d.jhi[b] - (FOLDOWN - 1)) : d.jhi[b] + 1;   // first row of the fold windows
        if (top && d.jhi[b] - d.jlo[b] + 1 < 3) { why = "a block at the fold has fewer than three rows"; return false; }
        for (int j0 = d.jlo[b]; j0 <= d.jhi[b]; j0 = (j0 < jtop && j0 + OWN >= jtop) ? jtop : j0 + OWN) {
            const bool fw = top && j0 == jtop;
            const int jmax = fw ? d.jhi[b] : std::min(j0 + OWN - 1, jtop - 1);
            const int tf = fw ? 2 + (d.jhi[b] - j0) : 0;
            for (int i0 = d.ilo[b]; i0 <= d.ihi[b]; i0 += OWN) {
                const long G0 = (long)d.iglob0[b] + (i0 - 2 - d.ilo[b]);
                const long G0m = (long)NX - G0 - 15;
                const int32_t dead = (int32_t)(-1 - (b * plane + (long)(j0 - 1) * nxb + (i0 - 1)));
                for (int ty = 0; ty <= X; ++ty)
                    for (int tx = 0; tx <= X; ++tx) {
                        if (!fw || ty <= tf) { tab.push_back((int32_t)W.at(b, i0 - 2 + tx, j0 - 2 + ty)); continue; }
                        if (ty > tf + 3) { tab.push_back(dead); continue; }
                        const int jg = NY - (tf + 3 - ty), ig = wrap(G0m + tx);
                        const int32_t c = jg >= 1 ? cell[(size_t)(jg - 1) * NX + (ig - 1)] : -1;
                        if (c < 0) { why = "a cell mirrored across the fold is not on this rank"; return false; }
                        tab.push_back(c);
                    }
                tiles.push_back(b); tiles.push_back(i0); tiles.push_back(j0);
                tiles.push_back((fw ? 1 : 0) | (tf << 8) | (jmax << 16));
                tiles2.push_back((int32_t)G0); tiles2.push_back(NX); tiles2.push_back(0); tiles2.push_back(0);
            }
            if (fw) break;
        }
    }
    return true;
}
