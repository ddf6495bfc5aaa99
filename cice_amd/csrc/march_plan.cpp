// Host-only geometry and exchange plan of the marching path: see march_plan.h.
#include "march_plan.h"

#include <algorithm>
#include <map>

namespace {

struct Blk { int gi0, gj0, gnx, gny, owner; };

constexpr int PW = MARCH_PLAN_PAD;        // width of the overlap / the ring

// column x of a rank's rectangle (may lie up to P cells beyond it) -> (strip, lane) that holds it
inline void column_home(int x, int own, int nstrips, int &s, int &l)
{
    s = std::min(std::max(x, 0) / own, nstrips - 1);
    l = x - s * own + PW;
}

// duplicates of the owner lanes of a rank with `nxr` columns in strips of `own`: -1, or (strip << 8) | lane.
// false: some column would need two duplicates (then a narrower strip is tried)
bool dup_table(int nxr, int own, bool wrapx, std::vector<int32_t> &dup)
{
    const int ns = (nxr + own - 1) / own;
    dup.assign((size_t)ns * 64, -1);
    for (int sb = 0; sb < ns; ++sb) {
        const int cnt = std::min(own, nxr - sb * own);       // columns strip sb owns: lanes P .. P+cnt-1
        for (int l = 0; l < 64; ++l) {
            if (l >= PW && l < PW + cnt) continue;             // an owner
            if (!(l < PW || l < 2 * PW + cnt)) continue;       // beyond the P overlap lanes: nothing reads it
            int x = sb * own - PW + l;
            if (wrapx) { if (x < 0) x += nxr; else if (x >= nxr) x -= nxr; }
            if (x < 0 || x >= nxr) continue;                 // a halo column beyond the rectangle: filled by the exchange
            const int so = x / own, lo = PW + x % own;        // its owner
            int32_t &slot = dup[(size_t)so * 64 + lo];
            if (slot != -1) return false;
            slot = (sb << 8) | l;
        }
    }
    return true;
}

}  // namespace

bool build_march_fold(const cice_evp_hip_dims &d, int ext, int tyb, MarchFold &F, bool several_ranks)
{
    F = MarchFold();
    const int NY = d.ny_global;
    if (d.ns_boundary_type != CICE_EVP_BND_TRIPOLE && d.ns_boundary_type != CICE_EVP_BND_TRIPOLET) { F.error = "no tripole fold"; return false; }
    if (d.nranks > 1 && !several_ranks) { F.error = "tripole grid on several ranks: the fold band of the marching path is built for one rank"; return false; }
    if (d.nranks > 1 && (d.gj0 == nullptr || d.nblocks_tot <= 0)) { F.error = "global block table required when nranks > 1"; return false; }
    if (ext < 0 || (ext & 1)) { F.error = "ext must be even and >= 0"; return false; }
    if (tyb < 2 || tyb > 9) tyb = 5;
    F.ext = ext;
    F.trow = tyb - 1;
    const int ring = ext + PW;
    // tripoleT: the top physical row holds images (its T-cell areas are not dxT * dyT in CICE's arrays, which the marching kernel
    // would use): the zone's ring stays below it, the band is one row taller
    const int top = d.ns_boundary_type == CICE_EVP_BND_TRIPOLET ? 1 : 0;
    int row0 = NY - top - 2 * ring;                 // first row of the list with the smallest band, H = ext + P (+ 1)
    if (row0 < 0) { F.error = "grid too short for a marched zone under the fold band"; return false; }
    // down to a tile row of the block that holds it (the highest such row if blocks with different origins hold it)
    // Several ranks: one band for the whole grid, and NO snap -- the tile height is tuned by timing on each rank for itself
    // (evp_host_resident.cpp: tune_after_upload), so it is no input that every rank shares; each rank's tile list then starts with
    // the tile row of its own kernel that holds list_row0, and the rows below it that those tiles also run are spent like the rest.
    int snapped = -1;
    for (int b = 0; b < d.nblocks && d.nranks <= 1; ++b) {
        const int gj0 = d.jglob0[b] - 1, gny = d.jhi[b] - d.jlo[b] + 1;
        if (row0 < gj0 || row0 >= gj0 + gny) continue;
        snapped = std::max(snapped, gj0 + ((row0 - gj0) / F.trow) * F.trow);
    }
    if (snapped >= 0) row0 = snapped;
    F.list_row0 = row0;
    F.zone = row0 + ring;
    F.H = NY - F.zone;
    F.to_block[0] = F.zone - ring; F.to_block[1] = F.zone;
    F.to_rect[0] = F.zone; F.to_rect[1] = F.zone + ring;
    if (F.zone < 1 || F.H < ring) { F.error = "grid too short for a marched zone under the fold band"; return false; }
    return true;
}

void march_fold_tile_rows(const MarchFold &F, int gj0, int gny, int &by0, int &by1)
{
    by0 = by1 = 0;
    if (gny <= 0 || gj0 + gny <= F.list_row0) return;            // the block lies below the list
    by0 = F.list_row0 > gj0 ? (F.list_row0 - gj0) / F.trow : 0;
    by1 = (gny - 1) / F.trow + 1;                                 // (its last tile row also owns the T-row jhi + 1)
}

bool build_march_plan(const cice_evp_hip_dims &d, int own_max, bool wrap_inside, int ext, MarchPlan &P, int fold_h, const MarchFold *ranks_fold)
{
    P = MarchPlan();
    const int me = d.rank;
    const int NX = d.nx_global, NY = d.ny_global;
    if (d.nghost != 1) { P.error = "nghost != 1"; return false; }
    const bool tripole = d.ns_boundary_type == CICE_EVP_BND_TRIPOLE || d.ns_boundary_type == CICE_EVP_BND_TRIPOLET;
    if (tripole && d.nranks > 1 && !ranks_fold) {
        P.error = "tripole grid on several ranks: the fold band of the marching path is built for one rank";
        return false;
    }
    if (d.ns_boundary_type == CICE_EVP_BND_CYCLIC || (tripole && fold_h <= 0) || (!tripole && fold_h > 0)) {
        P.error = "north-south boundary is not closed";
        return false;
    }
    if (fold_h >= NY) { P.error = "fold band as tall as the grid"; return false; }
    const bool ew_cyclic = d.ew_boundary_type == CICE_EVP_BND_CYCLIC;
    std::vector<Blk> blk;
    if (d.gi0 != nullptr && d.nblocks_tot > 0) {
        for (int k = 0; k < d.nblocks_tot; ++k) blk.push_back({d.gi0[k] - 1, d.gj0[k] - 1, d.gnx[k], d.gny[k], d.gowner[k]});
    } else {
        if (d.nranks != 1) { P.error = "global block table required when nranks > 1"; return false; }
        for (int b = 0; b < d.nblocks; ++b)
            blk.push_back({d.iglob0[b] - 1, d.jglob0[b] - 1, d.ihi[b] - d.ilo[b] + 1, d.jhi[b] - d.jlo[b] + 1, me});
    }
    const int nranks = std::max(1, (int)d.nranks);
    // Several ranks under ONE fold band (ranks_fold): the ranks whose blocks reach above the zone hold the band, each over its own
    // columns (P.top); the band's tile list (rows list_row0 .. NY - 1) must lie inside that top row of ranks.
    const bool shared = ranks_fold != nullptr && fold_h > 0 && nranks > 1;
    const int zone = NY - fold_h, fring = ext + PW;
    P.top.assign(nranks, 0);
    if (shared) {
        std::vector<int> uy0(nranks, 1 << 30), uy1(nranks, -1);
        for (const Blk &b : blk) {
            if (b.owner < 0) { P.error = "eliminated land blocks: the ranks' sub-domains are not rectangles"; return false; }
            if (b.owner >= nranks) { P.error = "block owner out of range"; return false; }
            uy0[b.owner] = std::min(uy0[b.owner], b.gj0); uy1[b.owner] = std::max(uy1[b.owner], b.gj0 + b.gny - 1);
        }
        for (int r = 0; r < nranks; ++r) {
            if (uy1[r] < 0) continue;
            P.top[r] = uy1[r] >= zone ? 1 : 0;
            // (the rule of the closed boundary below, with the zone's top in the boundary's place: the rank under a top rank holds
            // ext + P rows of it, and those must be rows of the zone.  list_row0 == zone - (ext + P), so this is also the test that
            // the rows of the band's tile list, list_row0 .. NY - 1, lie inside the top row of ranks: one refusal, one reason)
            if (P.top[r] && uy0[r] > 0 && uy0[r] > ranks_fold->list_row0) {
                P.error = "a top rank's share of the marched zone is thinner than its redundant rim + ring: the fold band's list rows "
                          "do not lie inside the top row of ranks";
                return false;
            }
        }
        for (char t : P.top) P.band_ranks += t;
    } else if (fold_h > 0) {
        P.top[std::min(std::max(me, 0), nranks - 1)] = 1;
        P.band_ranks = 1;
    }
    if (fold_h > 0) {
        // the zone of a folded grid: the blocks cut off at row NY - fold_h (what lies above belongs to the band)
        std::vector<Blk> cut;
        for (Blk b : blk) {
            if (b.gj0 >= NY - fold_h) continue;
            b.gny = std::min(b.gny, NY - fold_h - b.gj0);
            cut.push_back(b);
        }
        blk.swap(cut);
    }
    // every rank's rectangle
    P.all.assign(nranks, MarchRect());
    std::vector<long> area(nranks, 0);
    std::vector<int> x0(nranks, 1 << 30), y0(nranks, 1 << 30), x1(nranks, -1), y1(nranks, -1);
    for (const Blk &b : blk) {
        if (b.owner < 0) { P.error = "eliminated land blocks: the ranks' sub-domains are not rectangles"; return false; }
        if (b.owner >= nranks) { P.error = "block owner out of range"; return false; }
        area[b.owner] += (long)b.gnx * b.gny;
        x0[b.owner] = std::min(x0[b.owner], b.gi0); y0[b.owner] = std::min(y0[b.owner], b.gj0);
        x1[b.owner] = std::max(x1[b.owner], b.gi0 + b.gnx - 1); y1[b.owner] = std::max(y1[b.owner], b.gj0 + b.gny - 1);
    }
    own_max = std::min(64 - 2 * PW, std::max(4, own_max));
    for (int r = 0; r < nranks; ++r) {
        if (area[r] == 0) continue;
        MarchRect &R = P.all[r];
        R.gx0 = x0[r]; R.gy0 = y0[r]; R.nxr = x1[r] - x0[r] + 1; R.nyr = y1[r] - y0[r] + 1;
        if ((long)R.nxr * R.nyr != area[r]) { P.error = "a rank's blocks do not tile a rectangle"; return false; }
        if (R.nxr < 4 || R.nyr < 1) { P.error = "a rank's rectangle is too small"; return false; }
        R.ok = true;
    }
    if (!P.all[me].ok) { P.error = "this rank holds no blocks"; return false; }
    if (ext < 0 || (ext & 1)) { P.error = "ext must be even and >= 0"; return false; }
    // the rectangle a rank holds = its own cells + ext on every side with a neighbour (the same rule for every rank)
    struct Held { MarchRect E; int w, e, s, n; bool wrap; };
    auto held = [&](int r) -> Held {
        const MarchRect &R = P.all[r];
        Held H{R, 0, 0, 0, 0, false};
        H.wrap = wrap_inside && ew_cyclic && R.nxr == NX;                   // wraps inside: no neighbour in x
        if (!H.wrap) {
            if (R.gx0 > 0 || ew_cyclic) H.w = ext;
            if (R.gx0 + R.nxr < NX || ew_cyclic) H.e = ext;
        }
        if (R.gy0 > 0) H.s = ext;
        if (R.gy0 + R.nyr < NY) H.n = ext;
        H.E.gx0 = R.gx0 - H.w; H.E.gy0 = R.gy0 - H.s;
        H.E.nxr = R.nxr + H.w + H.e; H.E.nyr = R.nyr + H.s + H.n;
        return H;
    };
    // A neighbour between a rank and a CLOSED boundary must be wide enough for the rim and its P-cell ring: otherwise the
    // held rectangle reaches past the global boundary, those positions stay zero here while the owner advances its cells
    // from the caller's boundary ghost values (rect_to_block) -- different operands for the same cell.  Such a layout is
    // refused (the one-subcycle kernels run it); every rank reaches the same verdict from the same table.
    for (int r = 0; r < nranks; ++r) {
        if (!P.all[r].ok) continue;
        const MarchRect &R = P.all[r];
        const int dw = R.gx0, de = NX - (R.gx0 + R.nxr), ds = R.gy0, dn = NY - (R.gy0 + R.nyr);
        const bool thin_x = !ew_cyclic && ((dw > 0 && dw < ext + PW) || (de > 0 && de < ext + PW));
        const bool thin_y = (ds > 0 && ds < ext + PW) || (dn > 0 && dn < ext + PW);
        if (thin_x || thin_y) {
            P.error = "a rank lies closer to a closed boundary than its redundant rim + ring is wide";
            return false;
        }
    }
    const Held HM = held(me);
    P.owned = P.all[me];
    P.me = HM.E;
    P.ext_w = HM.w; P.ext_e = HM.e; P.ext_s = HM.s; P.ext_n = HM.n;
    P.wrapx = HM.wrap;
    // strips: the widest `own` for which every column of this rank has at most one duplicate -- and the last strip
    // holds at least P columns: with fewer, the first columns BEYOND the rectangle (which the exchange fills)
    // would sit in two strips, as overlap lanes of the last but one and of the last, and a received cell has one home
    // (column_home) plus the duplicate of a column inside the rectangle only
    bool found = false;
    for (int own = own_max; own >= 4 && !found; --own) {
        const int ns = (P.me.nxr + own - 1) / own;
        if (ns > 1 && P.me.nxr - (ns - 1) * own < PW) continue;
        if (dup_table(P.me.nxr, own, P.wrapx, P.dup)) { P.me.own = own; found = true; }
    }
    if (!found) { P.error = "no strip width gives every column a single duplicate"; return false; }
    P.me.nstrips = (P.me.nxr + P.me.own - 1) / P.me.own;

    // (under a shared fold band the table is seen uncut up to row zone + ring: the ext + P columns a top rank holds beyond its own go on
    // above the zone, where they are rows of its x-neighbour's band -- which that rank has gathered into its rectangle, at these very
    // positions, before the ring travels: the corner cells)
    auto owner_of = [&](int gx, int gy) -> int {
        for (int r = 0; r < nranks; ++r) {
            const MarchRect &R = P.all[r];
            if (!R.ok || gx < R.gx0 || gx >= R.gx0 + R.nxr || gy < R.gy0) continue;
            if (gy < R.gy0 + R.nyr || (shared && P.top[r] && gy < zone + fring)) return r;
        }
        return -1;
    };
    std::map<int, MarchPeer> peers;
    const MarchRect &M = P.me;
    for (int D = 0; D < nranks; ++D) {
        if (!P.all[D].ok) continue;
        const Held HD = held(D);
        const MarchRect &E = HD.E;                                          // what D holds; its own cells start at (HD.w, HD.s)
        for (int y = -PW; y < E.nyr + PW; ++y)
            for (int x = -PW; x < E.nxr + PW; ++x) {
                const bool own_cell = x >= HD.w && x < E.nxr - HD.e && y >= HD.s && y < E.nyr - HD.n;
                if (own_cell) continue;
                int gx = E.gx0 + x;
                const int gy = E.gy0 + y;
                if (gy < 0 || gy >= NY) continue;                          // closed north / south
                // above D's own columns lies D's own band: gathered from its block layout, never exchanged
                if (shared && gy >= zone && x >= HD.w && x < E.nxr - HD.e) continue;
                if (gx < 0 || gx >= NX) {
                    if (!ew_cyclic) continue;
                    if (HD.wrap) continue;                                 // D reads those columns through the wrap of its strips
                    gx = ((gx % NX) + NX) % NX;
                }
                const int S = owner_of(gx, gy);
                if (S < 0) continue;
                if (D == me) {
                    MarchPeer &p = peers[S];
                    p.rank = S;
                    int s, l;
                    column_home(x, M.own, M.nstrips, s, l);
                    const int row = y + MARCH_PLAN_PAD;
                    p.recv_pos1.push_back((int32_t)(((long)row * M.nstrips + s) * 64 + l));
                    int32_t p2 = -1;
                    if (x >= 0 && x < M.nxr) {
                        const int32_t dd = P.dup[(size_t)s * 64 + l];
                        if (dd >= 0) p2 = (int32_t)(((long)row * M.nstrips + (dd >> 8)) * 64 + (dd & 255));
                    }
                    p.recv_pos2.push_back(p2);
                    p.recv_col.push_back(x);
                    p.recv_row.push_back(row);
                }
                if (S == me) {
                    MarchPeer &p = peers[D];
                    p.rank = D;
                    const int xs = gx - P.owned.gx0 + HM.w, ys = gy - P.owned.gy0 + HM.s;   // the source cell in what I hold
                    const int s = xs / M.own, l = PW + xs % M.own;
                    p.send_pos.push_back((int32_t)(((long)(ys + MARCH_PLAN_PAD) * M.nstrips + s) * 64 + l));
                    p.send_col.push_back(xs);
                }
            }
    }
    for (auto &kv : peers) {
        P.n_send += (int)kv.second.send_pos.size();
        P.n_recv += (int)kv.second.recv_pos1.size();
        P.peers.push_back(kv.second);
    }
    return true;
}

bool build_march_layout(const cice_evp_hip_dims &d, const MarchAsk &ask, MarchLayout &L)
{
    L = MarchLayout();
    MarchPlan &P = L.plan;
    MarchFold &F = L.fold;
    auto refuse = [&](const std::string &why) { L.why = why; return false; };
    // tripole grid: the rectangle is the zone under the fold band, whose height follows from the rim
    const bool tripole = d.ns_boundary_type == CICE_EVP_BND_TRIPOLE || d.ns_boundary_type == CICE_EVP_BND_TRIPOLET;
    // the rectangles of all ranks, this rank's strips and the exchange lists: the same verdict on every rank
    auto plan = [&](int e) -> bool {
        F = MarchFold();
        if (tripole && !build_march_fold(d, e, ask.tyb, F, true)) {
            P = MarchPlan();
            P.error = F.error;
            F = MarchFold();
            return false;
        }
        return build_march_plan(d, ask.own_max, ask.wrap_inside, e, P, F.H, &F);
    };
    // cells a rank holds beyond its own on every side with a neighbour: the ring of ext + P cells is then exchanged every
    // (ext + P)-th subcycle only (march_plan.h); 4 = after every second pass of four.  (Rounds 4-5, two subcycles per pass and a
    // two-cell ring, 3600 x 2400 as 4x2 pieces, one-GPU rehearsal: 54.3 / 52.3 / 52.0 / 51.2 us per subcycle with ext 0 / 2 / 4 / 6
    // against 47.0 without any exchange.)
    int ext = ask.ext == MARCH_ASK_UNSET ? -1 : std::max(0, ask.ext & ~1);
    if (ext >= 0) {
        if (!plan(ext)) return refuse(P.error);
    } else {
        // Default (round 6): the widest rim of 12 / 8 / 4 cells that costs no rank a strip more than a rim of 4 does and at most 2 %
        // more rows -- the exchange then comes every 16th / 12th / 8th subcycle for the same bytes per subcycle.  (The 8 x 1 pieces of
        // 3600 x 2400: 450 + 2 x 12 = 474 columns still fit the 9 strips that 458 need; measured on one GPU, ring exchanged with the
        // rank itself, an exchange costs ~38 us: 4.8 us per subcycle at every 8th.)  Every rank reaches the same value from the global
        // block table; a layout the plan refuses (a rank too thin next to a closed boundary) tries the next narrower rim.
        bool ok = false;
        std::string first_error;
        for (int e : {12, 8, 4, 0}) {
            if (!plan(e)) {
                if (first_error.empty()) first_error = P.error;
                continue;
            }
            bool fits = true;
            const bool ew_cyc = d.ew_boundary_type == CICE_EVP_BND_CYCLIC;
            for (const MarchRect &R : P.all) {
                if (!R.ok || e <= 4) continue;
                const bool span = ask.wrap_inside && ew_cyc && R.nxr == d.nx_global;      // wraps inside: no rim in x
                const int w = (R.gx0 > 0 || ew_cyc) ? 1 : 0, ea = (R.gx0 + R.nxr < d.nx_global || ew_cyc) ? 1 : 0;
                const int sn = R.gy0 > 0 ? 1 : 0, nn = R.gy0 + R.nyr < d.ny_global ? 1 : 0;
                const int own_eff = std::min(ask.own_max > 0 ? ask.own_max : MARCH_PLAN_OWN, MARCH_PLAN_OWN);
                const int w4 = R.nxr + (span ? 0 : 4 * (w + ea)), we = R.nxr + (span ? 0 : e * (w + ea));
                if ((we + own_eff - 1) / own_eff > (w4 + own_eff - 1) / own_eff) fits = false;
                if ((long)(R.nyr + e * (sn + nn)) * 100 > (long)(R.nyr + 4 * (sn + nn)) * 102) fits = false;
            }
            if (fits) { ext = e; ok = true; break; }
        }
        if (!ok) return refuse(first_error.empty() ? P.error : first_error);
    }
    L.ext = ext;
    L.ring_valid = ext + PW;
    // Subcycles per pass.  Round 6 measured what binds the kernel: a wave issues one instruction per 2.4 ns whatever it is, and a
    // row costs ~640 instructions per level plus ~350 that do not depend on the number of levels (loads, stores, addressing, the
    // register pipelines); a segment of sl rows marches sl + 2K - 1, the warm-up rows with part of the levels idle.  Measured on
    // the 8 x 1 and 4 x 2 pieces of 3600 x 2400 (22- and 20-row segments, profiles/r06_ring_rank.txt): 58.0 / 50.0 / 49.1 and
    // 54.9 / 46.8 / 46.0 us per subcycle with two / three / four subcycles per pass; 3600 x 2400 itself (160 rows) 362 / 315 / 293.
    // Four from 12 rows per segment, three from 8, two below.  Every rank must run the same passes (the ring is exchanged between
    // them), so the rule looks at the SHORTEST segment of any rank, which every rank works out from the global block table alone.
    // The test build can ask for a value.
    {
        int slmin = 1 << 30;
        for (const MarchRect &R : P.all) {
            if (!R.ok) continue;
            const int grow = d.nranks > 1 ? 2 * ext : 0;
            const int ns = (R.nxr + grow + MARCH_PLAN_OWN - 1) / MARCH_PLAN_OWN;
            const int nseg = std::max(1, 1024 / ns);
            slmin = std::min(slmin, std::max(6, (R.nyr + grow + nseg - 1) / nseg));
        }
        L.kpass = std::min(PW, slmin >= 12 ? 4 : slmin >= 8 ? 3 : 2);
    }
    if (ask.kpass != MARCH_ASK_UNSET) L.kpass = std::min(PW, std::max(2, ask.kpass));
    if (P.peers.size() > (size_t)MARCH_PLAN_MAXPEER) return refuse("more ring neighbours than the exchange lists hold");
    // blocks must tile [gx0, gx0+nxr) x [gy0, gy0+nyr) with full blocks of bsx x bsy (the last column / row may be smaller)
    auto bnx = [&](int b) { return d.ihi[b] - d.ilo[b] + 1; };
    auto bny = [&](int b) { return d.jhi[b] - d.jlo[b] + 1; };
    int gx0 = 1 << 30, gy0 = 1 << 30, gx1 = 0, gy1 = 0;
    for (int b = 0; b < d.nblocks; ++b) {
        gx0 = std::min(gx0, d.iglob0[b]); gy0 = std::min(gy0, d.jglob0[b]);
        gx1 = std::max(gx1, d.iglob0[b] + bnx(b) - 1); gy1 = std::max(gy1, d.jglob0[b] + bny(b) - 1);
    }
    const int nxr = gx1 - gx0 + 1, nyr = gy1 - gy0 + 1;
    int bsx = 0, bsy = 0;
    for (int b = 0; b < d.nblocks; ++b) {
        if (d.iglob0[b] == gx0) bsx = std::max(bsx, bnx(b));
        if (d.jglob0[b] == gy0) bsy = std::max(bsy, bny(b));
    }
    if (bsx <= 0 || bsy <= 0) return refuse("no block at the origin of the rectangle");
    const int nbx = (nxr + bsx - 1) / bsx, nby = (nyr + bsy - 1) / bsy;
    if ((long)nbx * nby != d.nblocks) return refuse("blocks do not tile a rectangle");
    L.blkid.assign((size_t)nbx * nby, -1);
    L.org.assign(d.nblocks, MarchOrg{0, 0});
    for (int b = 0; b < d.nblocks; ++b) {
        const int ox = d.iglob0[b] - gx0, oy = d.jglob0[b] - gy0;
        if (ox % bsx || oy % bsy) return refuse("block origins off the block grid");
        const int bi = ox / bsx, bj = oy / bsy;
        if (bnx(b) != std::min(bsx, nxr - ox) || bny(b) != std::min(bsy, nyr - oy)) return refuse("irregular block sizes");
        if (L.blkid[(size_t)bj * nbx + bi] >= 0) return refuse("two blocks at one place");
        L.blkid[(size_t)bj * nbx + bi] = b;
        L.org[b] = MarchOrg{ox + P.ext_w, oy + P.ext_s};        // block origins in the rectangle the rank HOLDS
    }
    // (the fold band: this rank's rows of it, and the ranks that hold some -- on several ranks only those whose blocks reach above the zone)
    L.band_rows = (F.H > 0 && !P.top.empty() && P.top[d.nranks > 1 ? d.rank : 0]) ? F.H : 0;
    L.band_ranks = P.band_ranks;
    if (nxr != P.owned.nxr || nyr - L.band_rows != P.owned.nyr || gx0 - 1 != P.owned.gx0 || gy0 - 1 != P.owned.gy0)
        return refuse("local blocks disagree with the global block table");
    L.bsx = bsx; L.bsy = bsy; L.nbx = nbx; L.nby = nby;
    const MarchRect &me = P.me;       // held: own cells + the redundant rim
    L.dup.assign(P.dup.size(), MARCH_PLAN_NODUP);
    for (size_t k = 0; k < P.dup.size(); ++k)
        if (P.dup[k] >= 0) L.dup[k] = (uint32_t)((((size_t)(P.dup[k] >> 8)) * MARCH_PLAN_S_NF * 64 + (P.dup[k] & 255)) * 8);
    L.ldx = ((me.nstrips * me.own + 64 + 2 * PW + 7) / 8) * 8;
    L.rows = me.nyr + 2 * PW + 3;      // y = -P .. nyr+P+2: halo, two rows the prefetch may touch, the dump row
    L.nblk = (size_t)L.rows * me.nstrips;
    if ((unsigned long long)L.nblk * MARCH_PLAN_S_NF * 512 >= (1ull << 32)) return refuse("state buffer beyond 32-bit byte offsets");
    // segments: one wave per SIMD (1024 of them), all resident at once -- measured at 3600 x 2400: 16 segments (960
    // waves) 318 us per subcycle, 24 (1440: some SIMDs get two) 400, 34 (2040: two each) 378, 12 (720) 372
    int seglen = ask.seglen;
    if (seglen <= 0) {
        // (medium domains, 0.45M .. 1M cells: shorter segments keep the count near 1000 -- 1080 x 720: 14-row segments 39 us
        // per subcycle against 53 for the one-subcycle kernel; each segment recomputes ~3.5 rows of warm-up)
        // (as many segments as fit 1024 waves: 3600 x 2400 has 60 strips -- 17 segments = 1020 waves = 255 workgroups, one per CU,
        // 302.8 us per subcycle; 16 segments (960 waves, 16 CUs idle) 310.1; 18 (1080: some SIMDs get two) 472 -- round 5, same box)
        const int want_seg = std::max(1, 1024 / me.nstrips);
        seglen = std::max(6, (me.nyr + want_seg - 1) / want_seg);
    }
    L.seglen = std::min(seglen, me.nyr);
    L.nseg = (me.nyr + L.seglen - 1) / L.seglen;
    L.nitems = L.nseg * me.nstrips;
    if (P.n_send + P.n_recv == 0) return true;
    // the ring: the peers' lists one after the other, and the same cells in the row-major byte mask
    for (size_t q = 0; q < P.peers.size(); ++q) {
        const MarchPeer &p = P.peers[q];
        L.cut_send[q] = (int)L.send_pos.size(); L.cut_recv[q] = (int)L.recv_pos1.size();
        L.send_pos.insert(L.send_pos.end(), p.send_pos.begin(), p.send_pos.end());
        L.recv_pos1.insert(L.recv_pos1.end(), p.recv_pos1.begin(), p.recv_pos1.end());
        L.recv_pos2.insert(L.recv_pos2.end(), p.recv_pos2.begin(), p.recv_pos2.end());
        for (size_t k = 0; k < p.send_pos.size(); ++k)
            L.send_midx.push_back((int32_t)((size_t)((p.send_pos[k] >> 6) / me.nstrips) * L.ldx + PW + p.send_col[k]));
        for (size_t k = 0; k < p.recv_pos1.size(); ++k)
            L.recv_midx.push_back((int32_t)((size_t)p.recv_row[k] * L.ldx + PW + p.recv_col[k]));
    }
    L.cut_send[P.peers.size()] = (int)L.send_pos.size(); L.cut_recv[P.peers.size()] = (int)L.recv_pos1.size();
    // Work items of the EARLY launch of an exchange pass (evp_host_march.cpp: march_run): per strip the rows that hold cells some
    // other rank receives, cut into short segments -- from the send lists themselves, so every sent cell is covered whatever the
    // layout.  Short segments (a third of the regular length, at least 6 rows) so that the launch, the pack and the
    // transfer end before the pass they overlap with does; each costs 2K - 1 rows of warm-up like any segment.  The pass
    // itself then runs over every OTHER (strip, row) of the rectangle (rest_items): the two launches of an exchange pass
    // store into disjoint cells (round-4 advice: they used to overlap on the band, storing the same bits twice).
    const int nstr = me.nstrips;
    std::vector<std::vector<char>> sent((size_t)nstr, std::vector<char>((size_t)me.nyr, 0));
    for (int pos : L.send_pos) {
        const int blk = pos >> 6, strip = blk % nstr, y = blk / nstr - PW;
        if (y >= 0 && y < me.nyr) sent[(size_t)strip][(size_t)y] = 1;
    }
    // runs of rows of one strip that are all sent (1) or all not (0), no longer than `most`
    auto runs = [&](char which, int most, std::vector<MarchItem> &items) {
        for (int st = 0; st < nstr; ++st)
            for (int y = 0; y < me.nyr;) {
                if (sent[(size_t)st][(size_t)y] != which) { ++y; continue; }
                int y1 = y;
                while (y1 < me.nyr && y1 - y < most && sent[(size_t)st][(size_t)y1] == which) ++y1;
                items.push_back(MarchItem{st, y, y1, 0});
                y = y1;
            }
    };
    runs(1, ask.bandseg > 0 ? ask.bandseg : std::max(6, L.seglen / 3), L.band_items);
    runs(0, L.seglen, L.rest_items);
    return true;
}

std::vector<MarchStep> march_schedule(int ndte, int kpass, int ring_valid, bool has_peers, bool fold)
{
    std::vector<MarchStep> steps;
    if (ndte <= 0 || kpass < 2) return steps;
    const int q = ndte / kpass;
    int rem = ndte % kpass;
    if (rem == 1) {
        steps.push_back(MarchStep{1, false, false, false});
        rem = 0;
    }
    const size_t first = steps.size();
    steps.insert(steps.end(), (size_t)q, MarchStep{kpass, false, false, false});
    if (rem) steps.push_back(MarchStep{rem, false, false, false});
    // (a pass advances the cells the rank holds -- its own + ext -- and only reads the P-cell ring around them: whatever is left of
    // the ring afterwards is a state older)
    int valid = ring_valid;          // cells beyond the rank's own that hold the current state (the gather's exchange just filled them)
    for (size_t k = first; k < steps.size(); ++k) {
        MarchStep &s = steps[k];
        s.last = k + 1 == steps.size();
        valid = std::min(valid - s.size, ring_valid - PW);
        const bool spent = !s.last && valid < steps[k + 1].size;
        s.exch = has_peers && (s.last || spent);
        s.fexch = fold && spent;
        if (s.exch || s.fexch) valid = ring_valid;
    }
    return steps;
}
