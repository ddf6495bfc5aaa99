// =====================================================================
// C-grid EVP subcycle behind the C ABI (include/cice_evp_hip.h, cice_evp_hip_cgrid_*): device state, ghost-image
// table, the tables of every schedule, upload / download, the preparation, what follows the loop, the read-outs.  The loop
// itself -- a captured graph of one (cg_one: one rank, no fold), three (fused schedule) or five launches per subcycle
// (evp_cgrid.hip) -- is evp_host_cgrid_loop.cpp; the state both share: evp_host_cgrid.h.
//
// Replaces evp()'s loop for grid_ice = 'C' (ice_dyn_evp.F90:938-1099).  The caller has run the reference's own
// preparation (dyn_prep1/2 at U, N and E points, seabed stress, the grid averages of the forcing) and hands over
// what the loop reads; it gets back what the loop writes.  Cyclic / closed / open boundaries; any number of blocks
// per rank (their ghost cells are images like any other).  Ghost cells that mirror cells of OTHER ranks are filled
// by the B-grid path's velocity exchange (halo_remote_pair: mailbox stores over xGMI, or RCCL point-to-point) run on
// pairs of the loop's arrays after the launch that produces them -- the same points at which the reference calls
// ice_HaloUpdate.  Tripole grids, u-fold and T-fold (tripoleT): a fold step per exchange point from host-built lists
// (halo_plan.cpp: build_fold_list).  Where the blocks next to the fold have more than one owner, every exchange goes
// through the C grid's own lists instead (HaloPlan::cg_peers): the ghost cells of the rows up to the fold and, behind them
// in the same exchange, the raw values the fold step of another rank reads, into staging slots behind the C-grid arrays.
// =====================================================================
#include <cmath>
#include <set>

#include "evp_host_cgrid.h"

namespace evp_host {
CGridState CG;

size_t cgrid_allocs() { return CG.mem.owned.size(); }

void cgrid_free()
{
    CG.mem.free_all();
    for (auto &kv : CG.graphs) (void)hipGraphExecDestroy(kv.second.exec);
    if (CG.side.st) (void)hipStreamDestroy(CG.side.st);
    if (CG.side.fork) (void)hipEventDestroy(CG.side.fork);
    if (CG.side.join) (void)hipEventDestroy(CG.side.join);
    CG = CGridState();
}

// ---- switches: each is read here and nowhere else (the loop's own: evp_host_cgrid_loop.cpp).  env_test(): the test build only (evp_host.h) ----
static bool split_faces_on() { return env_on(env_test("CICE_EVP_HIP_CGRID_SPLIT"), S.n <= 600000); }
static int xcd_switch() { return env_int(env_test("CICE_EVP_HIP_CGRID_XCD"), 1); }    // 0: plain 2-D launch, > 1: so many rows per band
static bool geo_switch() { return env_on(env_test("CICE_EVP_HIP_CGRID_GEO"), true); }
bool march_avgs_switch() { return env_on(env_test("CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH"), false); }   // =1: avg_strength on the marched split schedules
static int one_shape_switch(int dflt) { return std::min(2, std::max(0, env_int(env_test("CICE_EVP_HIP_CGRID_ONE_SHAPE"), dflt))); }
static int one_strip_switch() { return std::max(1, env_int(env_test("CICE_EVP_HIP_CGRID_ONE_STRIP"), 1 << 20)); }
static bool prof_on() { return env_on(env_test("CICE_EVP_HIP_CGRID_PROF"), false); }
static int strip_switch() { return env_int(env_test("CICE_EVP_HIP_CGRID_STRIP"), ENV_UNSET); }
static int strip_edge_switch() { return std::min(2, std::max(0, env_int(env_test("CICE_EVP_HIP_CGRID_STRIP_EDGE"), 0))); }
bool res_cull() { return env_on(env_test("CICE_EVP_HIP_CGRID_RES_CULL"), true); }
static bool res_sleep_on() { return env_on(env_test("CICE_EVP_HIP_CGRID_RES_SLEEP"), false); }
static int res_debug() { return env_int(env_test("CICE_EVP_HIP_CGRID_RES_DEBUG"), 0); }
static bool fast_switch() { return env_on(env_test("CICE_EVP_HIP_CGRID_FAST"), true); }
bool verbose() { return env("CICE_EVP_HIP_VERBOSE") != nullptr; }
// The marched kernel's knobs (cg_strip; test build): work items that fill the chip once, a forced segment length in rows (0: the
// planner's), whether the kernel may form six of the eight lengths itself, and -- several ranks -- slots left to the frame's workgroups
constexpr long STRIP_SLOTS = 2048;           // about two waves per SIMD resident at once (256 CUs x 8)
constexpr long STRIP_MIN_CELLS = 300000;     // the size rule: where the work items fill enough of the chip (measured: build_one_tables)
struct StripKnobs { long slots; int seg_forced; bool want_len; int reserve; };
static StripKnobs strip_knobs()
{
    const int seg = env_int(env_test("CICE_EVP_HIP_CGRID_STRIP_SEG"), ENV_UNSET);
    return {std::max(1, env_int(env_test("CICE_EVP_HIP_CGRID_STRIP_ITEMS"), (int)STRIP_SLOTS)), seg == ENV_UNSET ? 0 : std::max(1, seg),
            env_on(env_test("CICE_EVP_HIP_CGRID_STRIP_LEN"), true), env_int(env_test("CICE_EVP_HIP_CGRID_MARCH_RESERVE"), ENV_UNSET)};
}

// cg_one with 15 of its 23 static arrays derived in the kernel from the other eight (evp_cgrid.hip: DSlab): allowed when
// every identity holds bit for bit on the caller's arrays (derive_geometry_check, once per cice_evp_hip_cgrid_set_geometry).
// CICE_EVP_HIP_CGRID_GEO=0 keeps all 23 arrays in use.
bool geo_derived() { return CG.gmask && geo_switch(); }
void fill(EvpCgrid &A)
{
    const cice_evp_hip_params &q = S.prm;
    for (int k = 0; k < CG_NF; ++k) A.f[k] = CG.f[k];
    for (int k = 0; k < CG_NIN; ++k) A.in[k] = CG.in[k];
    for (int k = 0; k < CG_NG; ++k) A.g[k] = CG.g[k];
    A.gmask = geo_derived() ? CG.gmask : nullptr;
    A.gstride = S.n;
    A.strengthU = CG.strengthU;
    A.s12_in = nullptr;
    A.facE = CG.fac[0];
    A.facN = CG.fac[1];
    A.mask = CG.mask;
    A.img_slot = CG.img_slot;
    A.img_dst = CG.img_dst;
    A.blk = S.blk;
    A.p = {q.arlx1i, q.denom1, q.brlx, q.revp, q.e_factor, q.epp2i, q.capping, q.Ktens, q.u0, q.cosw, q.sinw, q.rhow};
    A.deltaminEVP = q.deltaminEVP;
    A.nx = S.d.nx_block;
    A.ny = S.d.ny_block;
    A.nblocks = S.d.nblocks;
    A.avg_strength = CG.avg_strength;
    A.tripole = CG.tripole ? 1 : 0;
    A.split_faces = split_faces_on();      // two waves per cell in the fused step kernel while the grid is small enough to be latency-bound
    {   // XCD-banded workgroup numbering (evp_cgrid.hip: cell())
        const int xcd = xcd_switch();
        const int gy = (S.d.ny_block + 3) / 4;      // TY = 4 rows per workgroup
        const int gx = (S.d.nx_block + 63) / 64;    // TX = 64
        A.xcd_rows = xcd ? std::min((gy + 7) / 8, xcd > 1 ? xcd : std::max(1, 256 / gx)) : 0;
    }
    A.plane = S.plane;
}

bool remote() { return !S.plan.peers.empty() || !S.plan.cg_peers.empty(); }
// the blocks next to the tripole fold have more than one owner: the C grid's exchange (ghost cells + fold sources into
// staging slots n + t of every exchanged array) replaces the velocity lists at every exchange point
bool fold_exchange() { return CG.tripole && S.plan.cg_split; }
// length of an exchanged array: the rank's cells and, where the fold rows have several owners, the staging slots of the fold exchange
size_t field_len() { return S.n + (fold_exchange() ? (size_t)S.plan.cg_tail : 0); }
// ghost cells owned by other ranks, for two of the loop's arrays (no-op on one rank).  Every exchange inside the loop
// goes through the masked halo when the host has handed one over (maskhalo_dyn: evp() builds it for the C grid as the
// five-point dilation of iceTmask, ice_dyn_evp.F90:739-770, and passes halo_info_mask to every dyn_haloUpdate of the
// loop, :965-1096: masked = true); copies inside a rank -- the pushes of the kernels -- are never masked, as in ice_HaloMask.
int exchange(double *a, double *b, bool masked)
{
    if (fold_exchange()) return cgrid_fold_exchange(a, b, field_len());
    return remote() ? halo_remote_pair(a, b, masked) : 0;
}

// the fold step of up to four fields (FoldField: evp_host_cgrid.h)
void fold(const FoldField *fs, int n)
{
    if (!CG.tripole) return;
    EvpCgFold F{};
    for (const FoldField *f = fs; f < fs + n; ++f) {
        F.x[F.nfields] = f->x;
        F.loc[F.nfields] = f->loc;
        F.isign[F.nfields] = f->vec ? -1.0 : 1.0;
        ++F.nfields;
    }
    for (int l = 0; l < 4; ++l) F.L[l] = {CG.fold[l].dst, CG.fold[l].a, CG.fold[l].b, CG.fold[l].flip, CG.fold[l].n};
    F.tmp = CG.fold_tmp;
    F.maxn = CG.fold_maxn;
    evp_launch_cgrid_fold(F, S.stream);
}


// Checks, on every cell the kernels can read (the blocks' cells with their ghost ring; the ratios and nothing else need
// a neighbour: interior cells), that the caller's derived arrays are what the reference's start-up computes from dx / dy
// (the list: evp_cgrid.hip above DSlab).  Compared as BITS.  Returns the four masks as bits, or an empty vector + why.
// areas = false: the land masks and the boundary ratios only (what the on-chip resident kernel derives on a tripole grid).
// jmax (may be null): per block the last row the identities have to hold on (the marched kernel under a fold band derives nothing
// above it: on the ghost row beyond the fold they do not hold and need not); the boundary ratios, which take a length of the row to
// the north, up to the row below it; a block with jmax < 1 is not looked at.  Cells not looked at get no mask bits.
static std::vector<uint8_t> derive_geometry_check(const double *const *g, std::string &why, bool areas = true, const std::vector<int> *jmax = nullptr)
{
    const int nxb = S.d.nx_block;
    std::vector<uint8_t> gm(S.n, 0);
    auto same = [](double a, double b) { return std::memcmp(&a, &b, 8) == 0; };
    auto bad = [&](const char *what, int b, int i, int j) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "%s differs from the reference's start-up formula at block %d cell (%d, %d)", what, b, i, j);
        why = buf;
        return std::vector<uint8_t>();
    };
    const double dmin = S.prm.deltaminEVP;
    for (int b = 0; b < S.d.nblocks; ++b)
        for (int j = S.jlo[b] - 1; j <= (jmax ? std::min((*jmax)[b], S.jhi[b] + 1) : S.jhi[b] + 1); ++j)
            for (int i = S.ilo[b] - 1; i <= S.ihi[b] + 1; ++i) {
                const size_t p = (size_t)b * S.plane + (size_t)(j - 1) * nxb + (i - 1);
                const double ta = g[CG_DXT][p] * g[CG_DYT][p], ua = g[CG_DXU][p] * g[CG_DYU][p];
                const double na = g[CG_DXN][p] * g[CG_DYN][p], ea = g[CG_DXE][p] * g[CG_DYE][p];
                if (areas) {
                    if (!same(ta, g[CG_TAREA][p])) return bad("tarea", b, i, j);
                    if (!same(ua, g[CG_UAREA][p])) return bad("uarea", b, i, j);
                    if (!same(na, g[CG_NAREA][p])) return bad("narea", b, i, j);
                    if (!same(ea, g[CG_EAREA][p])) return bad("earea", b, i, j);
                    if (!same(ea > 0.0 ? 1.0 / ea : 0.0, g[CG_EAREAR][p])) return bad("earear", b, i, j);
                    if (!same(na > 0.0 ? 1.0 / na : 0.0, g[CG_NAREAR][p])) return bad("narear", b, i, j);
                    if (!same(dmin * ta, g[CG_DMINT][p])) return bad("DminTarea", b, i, j);
                }
                unsigned bits = 0;
                const int mk[4] = {CG_EPM, CG_NPM, CG_UVM, CG_HM};
                for (int q = 0; q < 4; ++q) {
                    const double m = g[mk[q]][p];
                    if (same(m, 1.0)) bits |= 1u << q;
                    else if (!same(m, 0.0)) return bad("a land mask (neither 0 nor 1)", b, i, j);
                }
                gm[p] = (uint8_t)bits;
                if (i >= S.ilo[b] && i <= S.ihi[b] && j >= S.jlo[b] && j <= S.jhi[b] && (!jmax || j < (*jmax)[b])) {
                    const double rx = -(g[CG_DXN][p + 1] / g[CG_DXN][p]), ry = -(g[CG_DYE][p + nxb] / g[CG_DYE][p]);
                    if (!same(rx, g[CG_RXN][p]) || !same(1.0 / rx, g[CG_RXNR][p])) return bad("ratiodxN / ratiodxNr", b, i, j);
                    if (!same(ry, g[CG_RYE][p]) || !same(1.0 / ry, g[CG_RYER][p])) return bad("ratiodyE / ratiodyEr", b, i, j);
                    // (finite and negative: the kernels put -1 in their place wherever the factor next to them is +0)
                    if (!(rx < 0.0 && ry < 0.0 && std::isfinite(rx) && std::isfinite(ry) && std::isfinite(1.0 / rx) && std::isfinite(1.0 / ry)))
                        return bad("a boundary ratio (not finite and negative)", b, i, j);
                }
            }
    return gm;
}

// The six lengths the reference's start-up forms from HTN (= dxN) and HTE (= dyE), BIT FOR BIT on every cell the marched kernel would
// form them for in the rectangle z (cgrid_plan.h: strip_len_range; false too where that cannot be verified)
static bool strip_lengths_hold(const StripZone &z, int EX, int EY, const double *const *g)
{
    auto same = [](double a, double b) { return std::memcmp(&a, &b, 8) == 0; };
    const int nxb = S.d.nx_block, nyb = S.d.ny_block;
    StripRange r;
    if (!strip_len_range(z, EX, EY, nxb, nyb, r)) return false;
    const double *N = g[CG_DXN], *E = g[CG_DYE];
    for (int j = r.j0; j <= r.j1; ++j)
        for (int i = r.i0; i <= r.i1; ++i) {
            const size_t p0 = (size_t)z.b * nxb * nyb + (size_t)(j - 1) * nxb + (i - 1);
            if (!(same(g[CG_DXU][p0], 0.5 * (N[p0] + N[p0 + 1])) && same(g[CG_DXT][p0], 0.5 * (N[p0] + N[p0 - nxb])) &&
                  same(g[CG_DXE][p0], 0.25 * (N[p0] + N[p0 + 1] + N[p0 - nxb] + N[p0 - nxb + 1])) &&
                  same(g[CG_DYU][p0], 0.5 * (E[p0] + E[p0 + nxb])) && same(g[CG_DYT][p0], 0.5 * (E[p0] + E[p0 - 1])) &&
                  same(g[CG_DYN][p0], 0.25 * (E[p0] + E[p0 - 1] + E[p0 + nxb] + E[p0 + nxb - 1]))))
                return false;
        }
    return true;
}


// Fold lists (halo_plan.cpp: build_fold_list) on the device
static int build_fold_lists()
{
    if (S.d.nx_global % 2) return fail(-4, "tripole: nx_global must be even");
    const cice_evp_hip_dims d = host_dims();
    CG.fold_maxn = 0;
    for (int loc = 0; loc < 4; ++loc) {
        FoldList L;
        if (S.plan.cg_split) L = S.plan.cg_fold[loc];      // (operands >= S.n: staging slots the exchange fills)
        else build_fold_list(d, loc, L);
        CGridState::Fold &Fd = CG.fold[loc];
        Fd.n = (int)L.dst.size();
        CG.fold_maxn = std::max(CG.fold_maxn, Fd.n);
        if (!Fd.n) continue;
        if (CG.mem.upload(Fd.dst, L.dst) || CG.mem.upload(Fd.a, L.a) || CG.mem.upload(Fd.b, L.b) || CG.mem.upload(Fd.flip, L.flip)) return -1;
    }
    if (CG.fold_maxn && CG.mem.alloc(CG.fold_tmp, (size_t)4 * CG.fold_maxn)) return -1;
    return 0;
}

// ---- what the marched kernel (cg_strip) and the kernels beside it need, whichever schedule runs them ----
static long interior_cells(const cice_evp_hip_dims &d)
{
    long n = 0;
    for (int b = 0; b < d.nblocks; ++b) n += (long)(d.ihi[b] - d.ilo[b] + 1) * (d.jhi[b] - d.jlo[b] + 1);
    return n;
}
// the kernel's 32-bit byte offsets span the static and the per-call table
static bool strip_offsets_fit() { return (double)S.n * 8.0 * std::max((int)CG_NG, (int)CG_NIN) < 4294967296.0; }
static int zeros(double *&p, size_t n) { return CG.mem.alloc(p, n, true); }      // a cleared array of doubles
// the second allocations of uvelE, vvelN, stresspT, stressmT (stress12U's always exists)
static int need_alt()
{
    for (int q = 0; q < 4; ++q)
        if (!CG.alt[q] && zeros(CG.alt[q], field_len())) return -1;
    return 0;
}
static int upload_items(MarchItems &M, const std::vector<int32_t> &items, int ex, int ey, int lengths, int seg, long cells)
{
    M.nitems = (int)(items.size() / 6);
    M.ex = ex; M.ey = ey;
    M.len = lengths;
    M.seg = seg;
    M.cells = cells;
    return CG.mem.upload(M.items, items);
}
// the plan's per-cell bits and workgroup lists of nlev levels, nscr scratch arrays, the second buffers, the side stream
static int upload_cell_lists(CellLists &Q, const std::vector<uint8_t> &cells, const std::vector<int32_t> *wg, int nlev, int nscr, long ncells)
{
    Q.ncells = ncells;
    if (CG.mem.upload(Q.cells, cells)) return -1;
    for (int k = 0; k < nlev; ++k) {
        Q.nwg[k] = (int)wg[k].size();
        if (CG.mem.upload(Q.wg[k], wg[k])) return -1;
    }
    for (int k = 0; k < nscr; ++k)
        if (zeros(Q.scr[k], S.n)) return -1;
    if (need_alt()) return -1;
    if (CG.side.st) return 0;           // (one second stream per geometry, whichever plans share it)
    HIPC(hipStreamCreateWithFlags(&CG.side.st, hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&CG.side.fork, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&CG.side.join, hipEventDisableTiming));
    return 0;
}

// Window table of the one-launch kernel: for every position of every window the cell whose value the reference has
// there.  Within one cell of the owned range that is the array cell itself -- interior cell, or the interior cell a ghost
// cell mirrors (halo plan), or the ghost cell marked static (nothing is copied into it); further out the walk goes on
// from the mirrored cell, neighbour by neighbour.
static int build_one_tables(const double *const *static23)
{
    const HaloPlan &P = S.plan;
    // the window: 32x8 on the smallest grids (more workgroups than 64x8 gives), 64x8 where that gives every CU one or two
    // workgroups (gx1: 462), 64x16 from there on -- the fewest recomputed positions and re-read rows per owned cell, which is
    // what counts once there are several windows per CU (720x270: 24.6 / 21.9 us with 32x8 / 64x16; 3600x2400: 1083 / 1032 /
    // 925 with 32x8 / 64x8 / 64x16).  CICE_EVP_HIP_CGRID_ONE_SHAPE=0 / 1 / 2 picks one
    const int shape = one_shape_switch(S.n > 160000 ? 2 : (S.n > 40000 ? 1 : 0));
    const int OX = shape ? 64 : 32, OY = shape == 2 ? 16 : 8;
    // Order of the windows = order of the workgroups on an XCD (each XCD takes a contiguous run of the list): row by row.
    // (Strips of a few windows in x, top to bottom, so that vertical neighbours run together and share their 2-3 common rows
    // in L2, were measured: 3600 x 2400 1083 us row by row, 1171 / 1139 / 1106 / 1082 in strips of 4 / 8 / 16 / 32 windows --
    // narrow strips cost more in DRAM locality than the shared rows save.  CICE_EVP_HIP_CGRID_ONE_STRIP=<n> for A/B.)
    const int strip = one_strip_switch();
    const cice_evp_hip_dims d = host_dims();
    std::vector<int32_t> tab, tiles;
    build_window_table(d, P, OX, OY, strip, tiles, tab);       // cgrid_plan.cpp (host only: CPU known-answer test)
    CGridState::One &O = CG.one;
    const bool ranks = remote();                 // no window kernel here: the table only tells which cells are regular
    if (!ranks) {
        O.ntiles = (int)(tiles.size() / 4);
        O.ox = OX;
        O.oy = OY;
        O.per_xcd = (O.ntiles + 7) / 8;
        if (CG.mem.upload(O.tab, tab) || CG.mem.upload(O.tiles, tiles) || need_alt()) return -1;
        if (prof_on() && CG.mem.alloc(O.prof, (size_t)O.ntiles * 8, true)) return -1;
    }
    // ---- the marched kernel's share (cg_strip): per block the rectangle its regular windows cover, if they form one ----
    // default: large domains (the rectangle at least 300 000 cells and half of the rank's); CICE_EVP_HIP_CGRID_STRIP=0 / 1 (test
    // build) switches it off / on wherever a regular window exists, CICE_EVP_HIP_CGRID_STRIP_SEG=<rows> sets the segment length
    {
        const int forced = strip_switch();
        int want = forced != ENV_UNSET ? (forced ? 1 : 0) : shape == 2 ? 2 : 0;              // 2: auto
        const long interior = interior_cells(d);
        if (want == 2 && interior < STRIP_MIN_CELLS) want = 0;
        // the windows cg_one keeps beside the marched kernel -- a frame one window deep along the block's edges -- are cut
        // smaller than the ones it covers a whole domain with: 32 x 8 positions (29 x 5 owned), 256 threads, four workgroups per CU
        // in one round instead of two rounds of 1024-thread ones (3600 x 2400: the frame 51 us -> see DESIGN.md section 7)
        const int eshape = strip_edge_switch();
        const int EX = eshape ? 64 : 32, EY = eshape == 2 ? 16 : 8;
        std::vector<int32_t> etiles, etab;
        if (want && (EX != OX || EY != OY)) {
            build_window_table(d, P, EX, EY, 1 << 20, etiles, etab);
            tiles.swap(etiles);
            tab.swap(etab);
        }
        const int nt = (int)(tiles.size() / 4), sx = EX - 3, sy = EY - 3;
        using Zone = StripZone;                        // (cgrid_plan.h: the planning is host-only code with a CPU test)
        std::vector<Zone> zones;
        long zcells = 0;
        std::vector<uint8_t> in_zone((size_t)nt, 0);
        if (!strip_offsets_fit()) want = 0;
        if (want) strip_zones(d, tiles, EX, EY, CG.h_img_slot.empty() ? nullptr : CG.h_img_slot.data(), zones);
        for (const Zone &z : zones) zcells += (long)(z.i1 - z.i0 + sx) * (z.j1 - z.j0 + sy);
        // (default: where the work items fill enough of the chip -- measured against cg_one alone: 720 x 270 23-48 us (segments of 4-16 rows)
        // against 22, 720 x 540 32 (8 rows) against 40, 1440 x 1080 95 against 154, 3600 x 2400 455-489 against 794)
        if (want == 2 && (2 * zcells < interior || zcells < STRIP_MIN_CELLS)) zones.clear();
        // The six lengths the reference's start-up forms from HTN (= dxN) and HTE (= dyE) -- dxU, dyU, dxT, dyT two-point means, dxE, dyN
        // four-point means (ice_grid.F90:3063-3280) -- checked BIT FOR BIT on every cell the marched kernel would form them for (each
        // rectangle with three columns and rows around it); where all hold the kernel forms them itself instead of loading them.  A
        // grid whose lengths were made otherwise (or a rectangle that reaches a row the reference extrapolates) keeps all eight loaded.
        const StripKnobs knobs = strip_knobs();
        bool lengths = !zones.empty() && static23 != nullptr && knobs.want_len;
        if (lengths) {
            auto holds = [&](const Zone &z) { return strip_lengths_hold(z, EX, EY, static23); };
            // (a rectangle whose outermost window row reaches a row the reference extrapolates -- j = 1, j = ny_global -- gives that
            // row of windows back to cg_one)
            std::vector<Zone> cut = zones;
            for (Zone &z : cut) {
                bool ok = false;
                for (int v = 0; v < 4 && !ok; ++v) {
                    Zone t = z;
                    if (v & 1) t.j1 -= sy;
                    if (v & 2) t.j0 += sy;
                    if (t.j1 < t.j0) continue;
                    if (holds(t)) { z = t; ok = true; }
                }
                lengths = lengths && ok;
            }
            if (lengths) {
                zones = cut;
                zcells = 0;
                for (const Zone &z : zones) zcells += (long)(z.i1 - z.i0 + sx) * (z.j1 - z.j0 + sy);
            }
        }
        if (!zones.empty()) {
            // strips of 60 owned columns (lanes 2 .. 61 of the wave; 59, lanes 3 .. 61, where the kernel forms the lengths; the last
            // strip of a rectangle is shifted west so that its lanes stay inside it and owns what is left); segments: about two
            // waves per SIMD resident at once over all strips (256 CUs x 8)
            // (measured, 3600 x 2400: 2006 items of 70 rows 567 us per subcycle; 2065 items -- 17 more than fit at once -- 693;
            // 2950 x 48 597, 4720 x 30 603, 11741 x 12 624: one round of work, as long as possible.  Shortest segment: 16 rows from a
            // million cells -- 1440 x 1080: 1608 items of 16 rows 95 us, 1992 of 13 104 --, 8 below -- 720 x 540: 804 items of 8 rows
            // 32 us, 408 of 16 49)
            long slots = knobs.slots;
            // (several ranks, A/B: so many of the resident slots left to the frame's workgroups, which run beside the marched kernel)
            if (ranks && knobs.reserve != ENV_UNSET) slots = std::max<long>(64, slots - std::max(0, knobs.reserve));
            std::vector<int32_t> items;
            const int seg = strip_items(zones, EX, EY, lengths ? 3 : 2, slots, zcells >= 1000000 ? 16 : 8, knobs.seg_forced, items);
            strip_windows(zones, tiles, in_zone);
            std::vector<int32_t> tiles_e, tab_e;
            const size_t per = (size_t)EX * EY;
            for (int w = 0; w < nt; ++w)
                if (!in_zone[(size_t)w]) {
                    tiles_e.insert(tiles_e.end(), tiles.begin() + 4 * w, tiles.begin() + 4 * w + 4);
                    tab_e.insert(tab_e.end(), tab.begin() + (size_t)w * per, tab.begin() + (size_t)(w + 1) * per);
                }
            if (ranks) {
                // the frame: every interior cell the items do not own, and where each level of the fused chain has to run for it
                CgFramePlan FP;
                std::string why;
                if (build_cg_frame(d, P, items, FP, why) != 1) return fail(-4, "C-grid EVP: %s", why.c_str());
                tiles_e.clear();
                tab_e.clear();
                if (upload_cell_lists(CG.fr, FP.cells, FP.wg, 3, 4, FP.rest_cells)) return -1;
            }
            if (upload_items(O.zone, items, EX, EY, lengths ? 1 : 0, seg, zcells)) return -1;
            O.ntiles_e = (int)(tiles_e.size() / 4);
            if (O.ntiles_e && (CG.mem.upload(O.tiles_e, tiles_e) || CG.mem.upload(O.tab_e, tab_e))) return -1;
        }
    }
    return 0;
}

// ---- tripole / tripoleT, one rank or several: what the marched kernel needs under the fold band, and the lists of the five phase
// kernels that advance every other interior cell -- across ranks the frame too (cgrid_plan.cpp: build_cg_march_fold plans and
// checks; enqueue_march_fold runs it).  Built only where the schedule can be used; a rank where no rectangle survives keeps the five
// full phases, with the reason in CG.mf.why.
static_assert(STRIP_AHEAD == EVP_CGSTRIP_AHEAD, "cgrid_plan.h and evp_device.h must agree on how far the marched kernel's loop runs ahead");
static int build_march_fold_tables(const double *const *static23)
{
    const HaloPlan &P = S.plan;
    CGridState::MarchFold &Q = CG.mf;
    const int want = cg_march_fold_wanted(sched_switches(), remote());    // (the rule the chooser applies: it reads the switches alone)
    if (!want) return 0;
    if (!strip_offsets_fit()) {
        Q.why = "the marched kernel's 32-bit offsets do not span the tables";
        return 0;
    }
    const cice_evp_hip_dims d = host_dims();
    const long interior = interior_cells(d);
    if (want == 2 && interior < STRIP_MIN_CELLS) {
        Q.why = "fewer cells than the marched kernel's size rule asks for";
        return 0;
    }
    constexpr int EX = 32, EY = 8, sy = EY - 3;
    // What the caller's static arrays allow for a rectangle: the 15 derived arrays on every row an item of it derives them for -- up to
    // two rows above its last owned one (earea of the row the N-face average takes), the boundary ratios one row less --, and the six
    // formed lengths (LEN).  Blocks are looked at one at a time: rows above the rectangle of a block at the fold need not hold.
    struct Geo : CgGeoCheck {
        const double *const *g;
        int operator()(const StripZone &z) const override
        {
            std::vector<int> jmax((size_t)S.d.nblocks, 0);
            jmax[(size_t)z.b] = z.j1 + sy - 1 + 2;
            std::string w;
            if (derive_geometry_check(g, w, true, &jmax).empty()) return 0;
            return strip_lengths_hold(z, EX, EY, g) ? 3 : 1;
        }
    } geo;
    geo.g = static23;
    const StripKnobs knobs = strip_knobs();
    CgMarchFoldPlan FP;
    const int rc = build_cg_march_fold(d, P, EX, EY, knobs.slots, 0, knobs.seg_forced, knobs.want_len ? 1 : 0, &geo, FP, Q.why);
    if (rc < 0) return fail(-4, "C-grid EVP: %s", Q.why.c_str());
    if (rc == 0) return 0;
    Q.by_size = 2 * FP.zone_cells >= interior && FP.zone_cells >= STRIP_MIN_CELLS;
    if (want == 2 && !Q.by_size) {
        Q.why = "the rectangles under the fold band are smaller than the marched kernel's size rule asks for";
        return 0;
    }
    // the land masks as bits, on the rows the items derive their geometry on
    std::vector<int> jmax((size_t)d.nblocks, 0);
    for (const StripZone &z : FP.zones) jmax[(size_t)z.b] = std::max(jmax[(size_t)z.b], z.j1 + sy - 1 + 2);
    std::string w;
    const std::vector<uint8_t> gm = derive_geometry_check(static23, w, true, &jmax);
    if (gm.empty()) return fail(-4, "C-grid EVP: fold-band plan: %s", w.c_str());
    // (the sixth scratch array, deltaU, only where visc_method = avg_strength may run this schedule)
    if (CG.mem.upload(Q.gmask, gm) || upload_cell_lists(Q.rest, FP.cells, FP.wg, 5, march_avgs_switch() ? 6 : 5, FP.rest_cells)) return -1;
    if (upload_items(CG.one.zone, FP.items, EX, EY, FP.lengths, FP.seg, FP.zone_cells)) return -1;
    Q.band_rows = FP.band_rows;
    Q.frame_cells = FP.frame_cells;
    return 0;
}

// ---- no fold, several ranks, visc_method = avg_strength on request: the same split with the frame as the whole REST
// (build_cg_march_fold's plan of a grid without a fold: no fold cells, no rows cut from the top).  Built where the fused chain's
// "zone marched + frame" has its plan (build_one_tables: the same switches and size rule) and the derived geometry holds on the
// whole rank; the size rule is applied to this plan's own zone as well.
static int build_march_frame_tables(const double *const *static23)
{
    CGridState::MarchFold &Q = CG.mf;
    if (!march_avgs_switch() || !CG.fr.cells || !CG.gmask || !strip_offsets_fit()) return 0;
    constexpr int EX = 32, EY = 8;
    struct Geo : CgGeoCheck {       // (the 15 derived arrays hold everywhere: CG.gmask; the six formed lengths per rectangle)
        const double *const *g;
        int operator()(const StripZone &z) const override { return strip_lengths_hold(z, EX, EY, g) ? 3 : 1; }
    } geo;
    geo.g = static23;
    const cice_evp_hip_dims d = host_dims();
    const StripKnobs knobs = strip_knobs();
    CgMarchFoldPlan FP;
    const int rc = build_cg_march_fold(d, S.plan, EX, EY, knobs.slots, 0, knobs.seg_forced, knobs.want_len ? 1 : 0, &geo, FP, Q.why);
    if (rc < 0) return fail(-4, "C-grid EVP: %s", Q.why.c_str());
    if (rc == 0) return 0;
    if (strip_switch() == ENV_UNSET && (2 * FP.zone_cells < interior_cells(d) || FP.zone_cells < STRIP_MIN_CELLS)) return 0;
    if (upload_cell_lists(Q.rest, FP.cells, FP.wg, 5, 6, FP.rest_cells) || upload_items(Q.zone, FP.items, EX, EY, FP.lengths, FP.seg, FP.zone_cells)) return -1;
    Q.frame_cells = FP.frame_cells;
    return 0;
}

// ---- the on-chip resident kernel (evp_cgrid_res.hip) ---------------------------------------------------------------
// Tables: cg_one's window table for 16 x 16 windows with one more row / column of positions, the map of cells some other
// window's rim mirrors (they publish a record every subcycle), the record buffers.  And the one property of the caller's
// static arrays the kernel relies on: it takes a NEIGHBOUR's operands from the cell the neighbouring position's value comes
// from, where the one-launch kernels read the array neighbour of the own cell -- the same thing if every ghost cell's static
// arrays are copies of its source's, which is checked here bit for bit on the sixteen arrays concerned (true of a grid whose
// static fields were halo-updated, as CICE's are; false, for instance, across a tripole fold).
static int build_res_tables(const double *const *static23)
{
    const HaloPlan &P = S.plan;
    CGridState::Res &Q = CG.res;
    Q.images_ok = true;
    const bool tripole = CG.tripole;
    for (size_t k = 0; k < P.local_dst.size() && Q.images_ok; ++k) {
        if (P.local_src[k] < 0) continue;
        if (tripole) {       // (the ghost row beyond the fold: by field location, below)
            const int db = (int)(P.local_dst[k] / S.plane);
            const int dj = (int)((P.local_dst[k] % S.plane) / S.d.nx_block) + 1;
            if (S.jglob0[db] + (dj - S.jlo[db]) > S.d.ny_global) continue;
        }
        // (the arrays the kernel reads at a NEIGHBOUR's position: the eight lengths, the four areas, the four land masks; the
        // reciprocal areas, DminTarea and the boundary ratios are read at the own cell only or not at all)
        for (int a : {CG_DXT, CG_DYT, CG_DXU, CG_DYU, CG_DXE, CG_DYE, CG_DXN, CG_DYN, CG_UAREA, CG_TAREA, CG_EAREA, CG_NAREA, CG_EPM, CG_NPM,
                      CG_UVM, CG_HM})
            if (std::memcmp(static23[a] + P.local_dst[k], static23[a] + P.local_src[k], sizeof(double)) != 0) {
                Q.images_ok = false;
                Q.why = "static array " + std::to_string(a) + " differs between ghost cell " + std::to_string(P.local_dst[k]) + " and its source";
                break;
            }
    }
    if (!Q.images_ok) return 0;
    const cice_evp_hip_dims d = host_dims();
    if (tripole) {
        // The kernel's FOLD variant takes the operands of a cell beyond the fold from the cell it mirrors: every ghost cell of the row
        // NY+1 must hold, array by array, what the cell its field location maps it to holds (true of a grid whose static fields went
        // through ice_HaloUpdate with their field_loc, as CICE's do).
        // (only the arrays the kernel reads THROUGH the remap: tarea, hm | uarea | dyE, earea, epm | dxN; everything else of a cell beyond
        // the fold is read from the array's own ghost row -- which need not be a mirror image: CICE computes e.g. dxE there from the ghost HTN)
        static const int by_loc[4][4] = {{CG_TAREA, CG_HM, -1, -1}, {CG_UAREA, -1, -1, -1}, {CG_DYE, CG_EAREA, CG_EPM, -1}, {CG_DXN, -1, -1, -1}};
        for (int loc = 0; loc < 4 && Q.images_ok; ++loc) {
            FoldList L;
            build_fold_list(d, loc, L);
            for (size_t k = 0; k < L.dst.size() && Q.images_ok; ++k) {
                if (L.b[k] != -1 || L.a[k] < 0 || L.a[k] == L.dst[k]) continue;      // (points ON the fold keep their own values)
                for (int a : by_loc[loc])
                    if (a >= 0 && std::memcmp(static23[a] + L.dst[k], static23[a] + L.a[k], sizeof(double)) != 0) {
                        Q.images_ok = false;
                        Q.why = "static array " + std::to_string(a) + " differs between the cell " + std::to_string(L.dst[k]) + " beyond the fold and the cell it mirrors";
                        break;
                    }
            }
        }
        if (!Q.images_ok) return 0;
    }
    constexpr int RX = 16, RY = 16, NPOS = (RX + 1) * (RY + 1);
    {   // a domain that can never be resident (3600 x 2400: 51k windows) gets no tables and no record buffers
        long nw = 0;
        for (int b = 0; b < S.d.nblocks; ++b)
            nw += (long)((S.ihi[b] - S.ilo[b] + RX - 3) / (RX - 3)) * ((S.jhi[b] - S.jlo[b] + RY - 3) / (RY - 3));
        if (nw > 16384) {     // (only the windows that hold ice have to be resident, per call: cg_res_live)
            Q.why = "more windows than can ever be resident at once (" + std::to_string(nw) + ")";
            return 0;
        }
    }
    std::vector<int32_t> tab, tiles, tiles2;
    if (tripole) {
        if (!build_fold_window_table(d, P, tiles, tiles2, tab, Q.why)) return 0;
        if ((long)tiles.size() / 4 > 16384) { Q.why = "more windows than can ever be resident at once"; return 0; }
        // the land masks as bits, the boundary ratios' identities (the five-phase kernels of these grids load all 23 arrays: no gmask yet)
        const std::vector<uint8_t> gm = derive_geometry_check(static23, Q.why, false);
        if (gm.empty()) return 0;
        if (CG.mem.upload(Q.gmask, gm) || need_alt()) return -1;
    } else {
        build_window_table(d, P, RX, RY, 1 << 20, tiles, tab, 1);
    }
    Q.ntiles = (int)(tiles.size() / 4);
    // the last owned row of a window, the last row of positions that matter to its owned cells (fold windows: the fold row)
    auto jmax_of = [&](int w) { return tripole ? tiles[4 * w + 3] >> 16 : S.jhi[tiles[4 * w]]; };
    // who publishes what, and is every hand-off mutual?  (cgrid_plan.cpp: cgres_dependencies -- the rule the kernel's ring applies)
    static_assert(CGRES_REACH == EVP_CGRES_REACH && CGRES_SLOTS == EVP_CGRES_SLOTS, "cgrid_plan.h and evp_device.h must agree on the windows' ring");
    std::vector<uint8_t> pub;
    {
        int n_edges = 0, n_oneway = 0;
        const int unsafe = cgres_dependencies(d, tripole, tiles, tab, &pub, &n_edges, &n_oneway);
        if (unsafe > 0) {
            // a window that is read by one it cannot be held back by within three subcycles could overwrite the record slot that
            // reader still waits for: static ineligibility (the one-launch kernel runs such a cut)
            Q.why = std::to_string(unsafe) + " of " + std::to_string(n_edges) + " hand-offs between windows have no chain back within " +
                    std::to_string(CGRES_SLOTS - 1) + " subcycles";
            return 0;
        }
    }
    // A neighbour's operands and state come from the cell the table names for the NEIGHBOURING POSITION; the one-launch kernels
    // (and the reference) read the array neighbour of the position's own cell.  Inside the domain the two are the same cell or an
    // image of it.  Outside a closed boundary they can be two different ghost cells (every block keeps its own): the kernel is
    // only right if both hold the same values -- the static arrays are compared here, the loop's state at every upload.
    {
        std::vector<int2> pairs;
        std::set<std::pair<int, int>> seen;
        const int nxb = S.d.nx_block;
        for (int w = 0; w < Q.ntiles && Q.images_ok; ++w) {
            // (tripole: a fold window's rows up to the fold row, the others' up to two rows beyond the last owned one)
            const int tymax = !tripole ? RY : (tiles[4 * w + 3] & 1) ? ((tiles[4 * w + 3] >> 8) & 255) + 1 : std::min(RY, jmax_of(w) - tiles[4 * w + 2] + 5);
            for (int ty = 0; ty < tymax; ++ty)
                for (int tx = 0; tx < RX; ++tx) {
                    const int a = tab[(size_t)w * NPOS + ty * (RX + 1) + tx];
                    if (a < 0) continue;                  // a position outside the domain computes nothing
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            if ((!dx && !dy) || tx + dx < 0 || ty + dy < 0 || ty + dy >= tymax) continue;
                            const int c = tab[(size_t)w * NPOS + (ty + dy) * (RX + 1) + (tx + dx)];
                            if (c >= 0) continue;         // inside the domain: the cell itself or an image of it
                            const int b = a + dx + dy * nxb, g = -1 - c;
                            if (b == g || !seen.insert({b, g}).second) continue;
                            pairs.push_back(make_int2(b, g));
                            for (int k : {CG_DXT, CG_DYT, CG_DXU, CG_DYU, CG_DXE, CG_DYE, CG_DXN, CG_DYN, CG_UAREA, CG_TAREA, CG_EAREA, CG_NAREA,
                                          CG_EPM, CG_NPM, CG_UVM, CG_HM})
                                if (std::memcmp(static23[k] + b, static23[k] + g, sizeof(double)) != 0) {
                                    Q.images_ok = false;
                                    Q.why = "static array " + std::to_string(k) + " differs between the ghost cells " + std::to_string(b) + " and " +
                                            std::to_string(g) + " outside the domain";
                                }
                        }
                }
        }
        if (!Q.images_ok) return 0;
        Q.npairs = (int)pairs.size();
        if (Q.npairs && CG.mem.upload(Q.pairs, pairs)) return -1;
    }
    if (CG.mem.upload(Q.tab, tab) || CG.mem.upload(Q.tiles, tiles) || CG.mem.upload(Q.pubmap, pub)) return -1;
    if (tripole && CG.mem.upload(Q.tiles2, tiles2)) return -1;
    if (CG.mem.alloc(Q.rec, (size_t)EVP_CGRES_SLOTS * S.n * 32, true) || CG.mem.alloc(Q.err, 8, true)) return -1;
    {   // until the first upload says otherwise: every window runs
        std::vector<int> ident(Q.ntiles);
        for (int w = 0; w < Q.ntiles; ++w) ident[w] = w;
        if (CG.mem.upload(Q.d_order, ident) || CG.mem.alloc(Q.live_win, ident.size()) || CG.mem.alloc(Q.live_cell, S.n)) return -1;
        HIPC(hipMemset(Q.live_cell, 1, S.n));
        Q.n_live = Q.ntiles;
    }
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, S.device));
    for (int v = 0; v < 8; ++v) Q.cap4[v] = (long)evp_cgrid_res_max_blocks_per_cu(v & 1, (v >> 1) & 1, tripole ? 1 : 0, v >> 2) * prop.multiProcessorCount;
    return 0;
}

int res_launch(const EvpCgrid &A, int nsub, bool dry, const PingPong &P)
{
    CGridState::Res &Q = CG.res;
    EvpCgRes R{};
    R.tab = Q.tab; R.tiles = Q.tiles; R.order = nullptr; R.ntiles = Q.ntiles;
    R.tiles2 = Q.tiles2; R.fold = CG.tripole ? 1 : 0;
    R.slow = CG.fast ? 0 : 1;
    R.long_sleep = res_sleep_on() ? 1 : 0;
    R.dbg = res_debug();
    // the windows that hold ice in this call (finish_upload: cg_res_live); CICE_EVP_HIP_CGRID_RES_CULL=0 (test build) runs them all
    if (res_cull()) {
        R.order = Q.d_order; R.ntiles = Q.n_live; R.live = Q.live_cell;
    }
    R.nsub = nsub; R.dry = dry ? 1 : 0;
    Q.epoch = (Q.epoch + 1u) & 0xFFFFFu;
    if (Q.epoch == 0) Q.epoch = 1;
    R.tag_base = Q.epoch << 12;
    R.par0 = Q.par;
    Q.par = (Q.par + nsub) & (EVP_CGRES_SLOTS - 1);
    R.spin_limit = (R.dbg & 16) ? 200000u : 4000000u;       // (the fault test need not wait seconds for the bound)
    R.err = Q.err;
    R.pubmap = Q.pubmap;
    for (int k = 0; k < EVP_CGRES_SLOTS; ++k) R.rec[k] = (char *)Q.rec + (size_t)k * S.n * 32;
    R.uE_in = P.cur[0]; R.vN_in = P.cur[1]; R.sp_in = P.cur[2]; R.sm_in = P.cur[3]; R.s12_in = P.cur[4];
    R.uE_out[0] = P.cur[0]; R.uE_out[1] = P.alt[0]; R.vN_out[0] = P.cur[1]; R.vN_out[1] = P.alt[1];
    R.sp_out[0] = P.cur[2]; R.sp_out[1] = P.alt[2]; R.sm_out[0] = P.cur[3]; R.sm_out[1] = P.alt[3];
    R.s12_out[0] = P.cur[4]; R.s12_out[1] = P.alt[4];
    R.gbase = CG.gslab; R.inbase = CG.inslab; R.stride = S.n;
    R.gmask = CG.tripole ? Q.gmask : CG.gmask;
    if (!dry && !Q.prof && prof_on() && CG.mem.alloc(Q.prof, (size_t)Q.ntiles * 32)) return -1;
    R.prof = dry ? nullptr : Q.prof;
    evp_launch_cgrid_res(A, R, S.stream);
    HIPC(hipGetLastError());
    Q.launched = true;
    return 0;
}

int res_check_error()
{
    CGridState::Res &Q = CG.res;
    if (!Q.launched) return 0;
    Q.launched = false;
    int ev[8] = {0};
    HIPC(hipMemcpy(ev, Q.err, sizeof ev, hipMemcpyDeviceToHost));
    if (ev[0]) {
        HIPC(hipMemset(Q.err, 0, sizeof ev));
        Q.mode = 0;
        return fail(-7, "resident C-grid kernel: a wait gave up (window %d, subcycle %d, cell %d, tag seen %#x, wanted %#x) -- workgroups not co-resident?",
                    ev[1], ev[2], ev[3], (unsigned)ev[4], (unsigned)ev[5]);
    }
    return 0;
}

int finish_upload(int32_t visc_method);


}  // namespace evp_host

using namespace evp_host;

extern "C" {

int cice_evp_hip_cgrid_set_geometry(const double *const *static23)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (!static23) return fail(-1, "null argument");
    const HaloPlan &P = S.plan;
    // (tripoleT: the same five launches + fold steps; only the fold lists differ -- all four locations rewrite the top
    // physical row there, halo_plan.cpp: build_fold_list_tfold)
    const bool tfold = S.d.ns_boundary_type == CICE_EVP_BND_TRIPOLET;
    const bool tripole = S.d.ns_boundary_type == CICE_EVP_BND_TRIPOLE || tfold;
    cgrid_free();
    CG.tripole = tripole;
    CG.tfold = tfold;
    // (the blocks next to the fold on several ranks: every exchanged array carries the staging slots of the fold exchange)
    const size_t nf = S.n + (tripole && P.cg_split ? (size_t)P.cg_tail : 0);
    for (auto &p : CG.f)
        if (zeros(p, nf)) return -1;
    if (zeros(CG.inslab, (size_t)CG_NIN * S.n) || zeros(CG.gslab, (size_t)CG_NG * S.n)) return -1;
    for (int k = 0; k < CG_NIN; ++k) CG.in[k] = CG.inslab + (size_t)k * S.n;
    for (int k = 0; k < CG_NG; ++k) {
        if (!static23[k]) return fail(-1, "null static array %d", k);
        CG.g[k] = CG.gslab + (size_t)k * S.n;
        if (h2d(CG.g[k], static23[k])) return -1;
    }
    if (zeros(CG.strengthU, S.n) || zeros(CG.alt[4], nf) || zeros(CG.fac[0], S.n) || zeros(CG.fac[1], S.n)) return -1;
    if (remote() && zeros(CG.umaskd, nf)) return -1;
    if (CG.mem.alloc(CG.d_flags, 1) || CG.mem.alloc(CG.mask, S.n) || CG.mem.alloc(CG.mask4, 4 * S.n)) return -1;
    // ghost images: for every interior cell the ghost cells of this rank that mirror it (what ice_HaloUpdate copies)
    CG.h_img_slot.assign(S.n, -1);
    std::vector<int> dst, zero;
    for (size_t k = 0; k < P.local_dst.size(); ++k) {
        const int src = P.local_src[k];
        if (tripole) {       // ghost row beyond the fold: location-dependent, done by the fold step, not by an image
            const int db = (int)(P.local_dst[k] / S.plane);
            const int dj = (int)((P.local_dst[k] % S.plane) / S.d.nx_block) + 1;
            if (S.jglob0[db] + (dj - S.jlo[db]) > S.d.ny_global - (tfold ? 1 : 0)) continue;    // (tripoleT: the top physical row too)
        }
        if (src < 0) {                              // neighbour block eliminated (land): the reference fills with zero
            zero.push_back(P.local_dst[k]);
            continue;
        }
        int &slot = CG.h_img_slot[src];
        if (slot < 0) {
            slot = (int)(dst.size() / 3);
            dst.insert(dst.end(), 3, -1);
        }
        int w = 0;
        while (w < 3 && dst[3 * slot + w] >= 0) ++w;
        if (w == 3) return fail(-4, "C-grid EVP: a cell with more than three ghost images");
        dst[3 * slot + w] = P.local_dst[k];
    }
    if (dst.empty()) dst.assign(3, -1);
    CG.h_img_dst = dst;
    if (CG.mem.upload(CG.img_slot, CG.h_img_slot) || CG.mem.upload(CG.img_dst, dst)) return -1;
    if (tripole && (P.fold_rows == 1 || P.cg_split))   // (ranks without the fold rows run the same schedule with empty lists)
        if (int rc = build_fold_lists()) return rc;
    if (!tripole && S.d.nx_block >= 3 && S.d.ny_block >= 3) {
        // (several ranks: the marched kernel's rectangles and the frame around them only -- no window runs there)
        if (int rc = build_one_tables(static23)) return rc;
        if (S.plan.peers.empty())
            if (int rc = build_res_tables(static23)) return rc;
    }
    if (tripole && !tfold && S.plan.peers.empty() && P.fold_rows == 1 && S.d.ew_boundary_type == CICE_EVP_BND_CYCLIC)
        if (int rc = build_res_tables(static23)) return rc;
    if (tripole && S.d.nx_block >= 3 && S.d.ny_block >= 3)
        if (int rc = build_march_fold_tables(static23)) return rc;
    if (!tripole) {      // (the five-phase kernels of tripole grids always load all 23)
        const std::vector<uint8_t> gm = derive_geometry_check(static23, CG.geo_why);
        if (!gm.empty()) {
            if (CG.mem.upload(CG.gmask, gm)) return -1;
            if (remote() && S.d.nx_block >= 3 && S.d.ny_block >= 3)
                if (int rc = build_march_frame_tables(static23)) return rc;
        } else if (verbose()) {
            std::fprintf(stderr, "[cice_evp_hip] C grid: all 23 static arrays stay in use: %s\n", CG.geo_why.c_str());
        }
    }
    CG.n_zero = (int)zero.size();
    if (CG.n_zero && CG.mem.upload(CG.zero_cells, zero)) return -1;
    HIPC(hipStreamSynchronize(S.stream));       // (the static arrays are on their way from the caller's)
    CG.geo = true;
    return 0;
}

int cice_evp_hip_cgrid_upload(const double *const *state14, const double *const *inputs23, const int32_t *iceTmask,
                              const int32_t *iceUmask, const int32_t *iceEmask, const int32_t *iceNmask,
                              int32_t visc_method)
{
    if (!S.ready || !CG.geo) return fail(-1, "C-grid EVP: geometry not set");
    if (!state14 || !inputs23 || !iceTmask || !iceUmask || !iceEmask || !iceNmask) return fail(-1, "null argument");
    if (visc_method != 0 && visc_method != 1) return fail(-1, "visc_method %d (0 avg_zeta, 1 avg_strength)", visc_method);
    CopyBatch B;
    for (int k = 0; k < 14; ++k) {
        if (!state14[k]) return fail(-1, "null state array %d", k);
        B.items.push_back({CG.f[k], state14[k]});
    }
    for (int k = 0; k < CG_NIN; ++k) {
        if (!inputs23[k]) return fail(-1, "null input array %d", k);
        B.items.push_back({CG.in[k], inputs23[k]});
    }
    if (h2d_batch(B)) return -1;
    // the mask byte is composed on the device from the caller's four logical arrays (bit5: iceU of an interior cell,
    // handed on to the ghost cells that mirror it -- the caller's iceUmask is not maintained on ghost cells: dyn_prep2
    // sets it on ilo..ihi x jlo..jhi only, ice_dyn_shared.F90:740-745)
    {
        const int32_t *m[4] = {iceTmask, iceUmask, iceEmask, iceNmask};
        for (int k = 0; k < 4; ++k)
            HIPC(hipMemcpyAsync(CG.mask4 + (size_t)k * S.n, m[k], S.n * sizeof(int32_t), hipMemcpyHostToDevice, S.stream));
        EvpCgrid A;
        fill(A);
        evp_launch_cgrid_mask(A, CG.mask4, S.stream);
    }
    return finish_upload(visc_method);
}

}  // extern "C"

namespace evp_host {
static unsigned g_last_call_flags = ~0u;        // the flag word of the last finish_upload as cg_call_setup left it (test build's read-out)
// what follows the arrival of the loop's inputs, however they arrived (cice_evp_hip_cgrid_upload: from the host;
// cice_evp_hip_cgrid_prep: computed here)
int finish_upload(int32_t visc_method)
{
    // evp() zeroes its work arrays at entry (ice_dyn_evp.F90:351-361)
    for (int k = CF_ZETA; k < CG_NF; ++k) HIPC(hipMemsetAsync(CG.f[k], 0, S.n * sizeof(double), S.stream));
    CG.avg_strength = visc_method;
    unsigned h_flags = ~0u;
    {
        EvpCgrid A;
        fill(A);
        HIPC(hipMemsetAsync(CG.d_flags, 0, sizeof(unsigned), S.stream));
        evp_launch_cgrid_call_setup(A, CG.fac[0], CG.fac[1], CG.d_flags, S.stream);
        if (CG.res.npairs) {
            const PingPong P;
            evp_launch_cgrid_res_pair_check(P.cur, CG.res.pairs, CG.res.npairs, CG.d_flags, S.stream);
        }
        HIPC(hipMemcpyAsync(&h_flags, CG.d_flags, sizeof(unsigned), hipMemcpyDeviceToHost, S.stream));
        if (CG.res.tab) {        // which windows of the resident kernel hold ice in this call
            CGridState::Res &Q = CG.res;
            HIPC(hipMemsetAsync(Q.live_cell, 0, S.n, S.stream));
            evp_launch_cgrid_res_live(A, Q.tab, Q.tiles, Q.ntiles, CG.tripole ? 1 : 0, Q.live_win, Q.live_cell, S.stream);
            Q.h_live.resize(Q.ntiles);
            HIPC(hipMemcpyAsync(Q.h_live.data(), Q.live_win, (size_t)Q.ntiles * sizeof(int), hipMemcpyDeviceToHost, S.stream));
        }
    }
    if (remote()) {                              // bit5 of ghost cells other ranks own
        EvpCgrid A;
        fill(A);
        evp_launch_cgrid_umask(A, CG.umaskd, 0, S.stream);
        if (int rc = exchange(CG.umaskd, CG.umaskd, false)) return rc;
        evp_launch_cgrid_umask(A, CG.umaskd, 1, S.stream);
    }
    if (visc_method == 1) {
        EvpCgrid A;
        fill(A);
        evp_launch_cgrid_phase(A, 5, 1, S.stream);
    }
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(S.stream));       // the caller may change its arrays after this returns
    CG.fast = (h_flags & 255u) == 0 && fast_switch();
    g_last_call_flags = h_flags;
    CG.res.pairs_state_ok = (h_flags & 256u) == 0;
    if (CG.res.tab) {
        CGridState::Res &Q = CG.res;
        std::vector<int> ord;
        for (int w = 0; w < Q.ntiles; ++w)
            if (Q.h_live[w]) ord.push_back(w);
        Q.n_live = (int)ord.size();
        if (Q.n_live) HIPC(hipMemcpy(Q.d_order, ord.data(), ord.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    CG.uploaded = true;
    CG.first = true;
    CG.mf.synced = false;
    CG.tail.strocn_ok = false;
    return 0;
}
}  // namespace evp_host

extern "C" {

int cice_evp_hip_cgrid_download(double *const *fields19)
{
    if (!CG.uploaded) return fail(-1, "C-grid EVP: nothing uploaded");
    if (!fields19) return fail(-1, "null argument");
    if (CG.res.launched) {       // a resident launch whose waits gave up has written nothing back: the caller's arrays stay untouched
        HIPC(hipStreamSynchronize(S.stream));
        if (int rc = res_check_error()) return rc;
    }
    if (fold_exchange() && S.direct.on) {        // a fold exchange whose wait gave up: nothing goes back to the caller
        HIPC(hipStreamSynchronize(S.stream));
        if (int rc = direct_check_error()) return rc;
    }
    CopyBatch B;
    for (int k = 0; k < CG_NF; ++k)
        if (fields19[k]) B.items.push_back({fields19[k], CG.f[k]});
    if (d2h_batch(B)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    float ms = 0;
    if (CG.t_nsub && hipEventElapsedTime(&ms, S.ev0, S.ev1) == hipSuccess) CG.t_loop_ms = ms;
    return 0;
}

// deformationsC_T (ice_dyn_shared.F90:1968-2074; evp() calls it right after the C-grid loop, ice_dyn_evp.F90:1106-1119) on
// the device, from the loop's resident final state: divu, shear, vort, rdg_conv, rdg_shear on the T-cells of dyn_prep2's
// list; the five arrays are inout (every other cell keeps the caller's value).  tarear: ice_grid's array, taken at the
// first call (NULL afterwards keeps it).
int cice_evp_hip_cgrid_deformations(const double *tarear, double *divu, double *shear, double *vort, double *rdg_conv,
                                    double *rdg_shear)
{
    if (!CG.uploaded) return fail(-1, "C-grid EVP: nothing uploaded");
    double *host[5] = {divu, shear, vort, rdg_conv, rdg_shear};
    for (double *p : host)
        if (!p) return fail(-1, "null argument");
    if (!CG.tarear) {
        if (!tarear) return fail(-1, "tarear needed on the first call");
        if (zeros(CG.tarear, S.n)) return -1;
    }
    if (tarear && h2d(CG.tarear, tarear)) return -1;
    CopyBatch U;
    for (int k = 0; k < 5; ++k) {
        if (!CG.post[k] && zeros(CG.post[k], S.n)) return -1;
        U.items.push_back({CG.post[k], host[k]});
    }
    if (h2d_batch(U)) return -1;
    EvpCgrid A;
    fill(A);
    evp_launch_cgrid_deformations(A, CG.tarear, CG.post[0], CG.post[1], CG.post[2], CG.post[3], CG.post[4], S.stream);
    HIPC(hipGetLastError());
    CopyBatch D;
    for (int k = 0; k < 5; ++k) D.items.push_back({host[k], CG.post[k]});
    if (d2h_batch(D)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

// dyn_finish at N and E points (ice_dyn_shared.F90:1291-1365; evp() calls it for both after the C-grid loop,
// ice_dyn_evp.F90:1408-1436) on the device, from the loop's resident final face velocities and the per-call operands the
// loop already holds (cdn_ocnX, aiX, uocnX, vocnX, fmX): the four arrays are inout -- written on the cells of dyn_prep2's
// N / E lists, every other cell keeps the caller's value.
int cice_evp_hip_cgrid_dyn_finish(double *strocnxN, double *strocnyN, double *strocnxE, double *strocnyE)
{
    if (!CG.uploaded) return fail(-1, "C-grid EVP: nothing uploaded");
    double *host[4] = {strocnxN, strocnyN, strocnxE, strocnyE};
    for (double *p : host)
        if (!p) return fail(-1, "null argument");
    CopyBatch U;
    for (int k = 0; k < 4; ++k) {
        if (!CG.post[k] && zeros(CG.post[k], S.n)) return -1;
        U.items.push_back({CG.post[k], host[k]});
    }
    if (h2d_batch(U)) return -1;
    EvpCgrid A;
    fill(A);
    evp_launch_cgrid_dyn_finish(A, 0, CG.post[0], CG.post[1], S.stream);
    evp_launch_cgrid_dyn_finish(A, 1, CG.post[2], CG.post[3], S.stream);
    HIPC(hipGetLastError());
    CopyBatch D;
    for (int k = 0; k < 4; ++k) D.items.push_back({host[k], CG.post[k]});
    if (d2h_batch(D)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

}  // extern "C"

namespace evp_host {
// ice_HaloUpdate(a, halo_info, loca, field_type_vector) and the same for b, on two arrays of field_len() doubles: every ghost
// cell this rank fills itself (the images, unconditionally; 0 next to an eliminated land block), the exchange with the other
// ranks over the UNMASKED lists -- the reference passes halo_info here, never halo_info_mask (ice_dyn_evp.F90:1437-1440,
// general/ice_step_mod.F90:1036-1039) --, the fold step of each location.  Ghost cells outside a closed or open boundary keep
// what they hold, as in ice_HaloUpdate (ice_boundary.F90:1178-1182: no fill there).  Collective wherever the loop's exchanges are.
static int tail_halo_pair(double *a, int loca, double *b, int locb)
{
    EvpCgrid A;
    fill(A);
    A.f[CF_UE] = a;      // (the image kernel addresses a field of the table: the pair stands in for two of them)
    A.f[CF_VN] = b;
    evp_launch_cgrid_phase(A, 9, CF_UE, S.stream);
    evp_launch_cgrid_phase(A, 9, CF_VN, S.stream);
    evp_launch_tail_zero_cells(a, b, CG.zero_cells, CG.n_zero, S.stream);
    if (int rc = exchange(a, b, false)) return rc;
    fold({{a, loca, true}, {b, locb, true}});
    HIPC(hipGetLastError());
    return 0;
}

// the loop's final state is there and no resident launch or fold exchange has given up on it
static int tail_state_ok()
{
    if (!CG.uploaded) return fail(-1, "C-grid EVP: nothing uploaded");
    if (CG.res.launched || (fold_exchange() && S.direct.on)) {
        HIPC(hipStreamSynchronize(S.stream));
        if (int rc = res_check_error()) return rc;
        if (int rc = direct_check_error()) return rc;
    }
    return 0;
}
}  // namespace evp_host

extern "C" {

// The end of evp() for grid_ice = 'C' (ice_dyn_evp.F90:1436-1443) on the loop's resident final state:
// (a) ice_HaloUpdate of strintxE (E face, vector) and strintyN (N face, vector) over the plain halo;
// (b) strintxU = grid_average_X2YS('N', strintxE, earea, epm), strintyU = grid_average_X2YS('E', strintyN, narea, npm)
//     (E2US / N2US, ice_grid.F90:3997-4004, 4290-4351): 0 everywhere, the quotient on the physical cells whose weights do not sum to 0.
// The device copies of strintxE / strintyN are the updated ones afterwards.  flags: reserved, 0.
int cice_evp_hip_cgrid_tail(double *strintxE, double *strintyN, double *strintxU, double *strintyU, int32_t flags)
{
    if (int rc = tail_state_ok()) return rc;
    if (flags != 0) return fail(-1, "cice_evp_hip_cgrid_tail: flags %d (reserved: 0)", (int)flags);
    for (auto &p : CG.tail.out)
        if (!p && zeros(p, S.n)) return -1;
    if (int rc = tail_halo_pair(CG.f[CF_STRX], 2, CG.f[CF_STRY], 3)) return rc;
    EvpTail G;
    fill_tail(G);
    evp_launch_tail_x2ys(G, CG.f[CF_STRX], CG.g[CG_EAREA], CG.g[CG_EPM], CG.tail.out[0], 1, S.stream);
    evp_launch_tail_x2ys(G, CG.f[CF_STRY], CG.g[CG_NAREA], CG.g[CG_NPM], CG.tail.out[1], 0, S.stream);
    HIPC(hipGetLastError());
    CopyBatch D;
    if (strintxE) D.items.push_back({strintxE, CG.f[CF_STRX]});
    if (strintyN) D.items.push_back({strintyN, CG.f[CF_STRY]});
    if (strintxU) D.items.push_back({strintxU, CG.tail.out[0]});
    if (strintyU) D.items.push_back({strintyU, CG.tail.out[1]});
    if (d2h_batch(D)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    if (fold_exchange() && S.direct.on)
        if (int rc = direct_check_error()) return rc;
    return 0;
}

// dyn_finish at U points, which evp() runs for grid_ice = 'C' too (ice_dyn_evp.F90:1395-1406; ice_dyn_shared.F90:1291-1365), from
// the loop's resident final uvel / vvel and iceUmask; the five U-point operands are the host's (the C-grid loop reads none of
// them): cdn_ocnU aiU uocnU vocnU fmU.  strocnxU / strocnyU inout: written on the ice U-cells only.  The device keeps the
// result and aiU for cice_evp_hip_cgrid_strocn_t.
int cice_evp_hip_cgrid_dyn_finish_u(const double *cdn_ocnU, const double *aiU, const double *uocnU, const double *vocnU,
                                    const double *fmU, double *strocnxU, double *strocnyU)
{
    if (int rc = tail_state_ok()) return rc;
    const double *host[5] = {cdn_ocnU, aiU, uocnU, vocnU, fmU};
    CGridState::Tail &T = CG.tail;
    if (!strocnxU || !strocnyU) return fail(-1, "null argument");
    CopyBatch U;
    for (int k = 0; k < 5; ++k) {
        if (!host[k]) return fail(-1, "null argument");
        if (!T.uin[k] && zeros(T.uin[k], S.n)) return -1;
        U.items.push_back({T.uin[k], host[k]});
    }
    for (auto &p : T.strocn)
        if (!p && zeros(p, S.n)) return -1;
    U.items.push_back({T.strocn[0], strocnxU});
    U.items.push_back({T.strocn[1], strocnyU});
    if (h2d_batch(U)) return -1;
    EvpTail G;
    fill_tail(G);
    evp_launch_tail_dyn_finish_u(G, CG.mask, 2u, S.prm.rhow, S.prm.cosw, S.prm.sinw, T.uin[0], T.uin[1], T.uin[2], T.uin[3], T.uin[4],
                                 CG.f[CF_UU], CG.f[CF_VU], T.strocn[0], T.strocn[1], S.stream);
    HIPC(hipGetLastError());
    CopyBatch D;
    D.items.push_back({strocnxU, T.strocn[0]});
    D.items.push_back({strocnyU, T.strocn[1]});
    if (d2h_batch(D)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    T.strocn_ok = true;
    return 0;
}

// strocn{x,y}T_iavg of step_dyn_horiz (general/ice_step_mod.F90:1012-1041) for grid_ice = 'C', as cice_evp_hip_strocn_t: from the
// strocnxU / yU and aiU cice_evp_hip_cgrid_dyn_finish_u left on the device, uarea / tarea of cice_evp_hip_cgrid_set_geometry; the
// NE-corner vector halo update through the loop's exchange of uvel / vvel and its fold step (unmasked).
int cice_evp_hip_cgrid_strocn_t(double *strocnxT_iavg, double *strocnyT_iavg)
{
    if (int rc = tail_state_ok()) return rc;
    CGridState::Tail &T = CG.tail;
    if (!T.strocn_ok) return fail(-1, "cice_evp_hip_cgrid_strocn_t: call cice_evp_hip_cgrid_dyn_finish_u first (its strocnxU / strocnyU stay on the device)");
    for (auto &p : T.work)
        if (!p && zeros(p, field_len())) return -1;
    for (auto &p : T.out)
        if (!p && zeros(p, S.n)) return -1;
    EvpTail G;
    fill_tail(G);
    evp_launch_tail_divide(G, T.strocn[0], T.strocn[1], T.uin[1], T.work[0], T.work[1], S.stream);
    if (int rc = tail_halo_pair(T.work[0], 1, T.work[1], 1)) return rc;
    evp_launch_tail_u2t_flux(G, T.work[0], T.work[1], CG.g[CG_UAREA], CG.g[CG_TAREA], T.out[0], T.out[1], S.stream);
    HIPC(hipGetLastError());
    CopyBatch D;
    if (strocnxT_iavg) D.items.push_back({strocnxT_iavg, T.out[0]});
    if (strocnyT_iavg) D.items.push_back({strocnyT_iavg, T.out[1]});
    if (d2h_batch(D)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    if (fold_exchange() && S.direct.on)
        if (int rc = direct_check_error()) return rc;
    return 0;
}

int cice_evp_hip_cgrid_sync(void)
{
    HIPC(hipStreamSynchronize(S.stream));
    float ms = 0;
    if (CG.t_nsub && hipEventElapsedTime(&ms, S.ev0, S.ev1) == hipSuccess) CG.t_loop_ms = ms;
    return res_check_error();
}

int cice_evp_hip_cgrid_run(int32_t ndte, int32_t visc_method, double *const *fields19, const double *const *inputs23,
                           const int32_t *iceTmask, const int32_t *iceUmask, const int32_t *iceEmask,
                           const int32_t *iceNmask)
{
    if (cice_evp_hip_cgrid_upload(fields19, inputs23, iceTmask, iceUmask, iceEmask, iceNmask, visc_method)) return -1;
    if (cice_evp_hip_cgrid_subcycle(ndte)) return -1;
    const int rc = cice_evp_hip_cgrid_download(fields19);
    if (rc == -7) {
        // The on-chip resident kernel gave up (a window was not resident: the GPU is not this rank's alone).  Its waits are
        // bounded, a launch that gives up writes nothing back and the download has not touched the caller's arrays: the call
        // is repeated from them with the per-subcycle kernels, which later calls use too (the verdict is kept).
        ++CG.res.fallbacks;
        if (verbose()) std::fprintf(stderr, "[cice_evp_hip] C grid: %s -- repeating the call without the resident kernel\n", g_err.c_str());
        g_err.clear();
        if (cice_evp_hip_cgrid_upload(fields19, inputs23, iceTmask, iceUmask, iceEmask, iceNmask, visc_method)) return -1;
        if (cice_evp_hip_cgrid_subcycle(ndte)) return -1;
        return cice_evp_hip_cgrid_download(fields19);
    }
    return rc;
}

// ---- the preparation phase on the device (SURVEY 8 f-2 for grid_ice = 'C'; kernels: evp_prep.hip prep1 / halo_center,
// evp_cgrid_prep.hip, evp_cgrid.hip cg_average) ----------------------------------------------------------------------
int cice_evp_hip_cgrid_set_prep_geometry(const int32_t *tmask, const int32_t *umaskCD, const int32_t *emask,
                                         const int32_t *nmask, const double *fcor_blk, const double *fcorE_blk,
                                         const double *fcorN_blk)
{
    if (!S.ready || !CG.geo) return fail(-1, "C-grid EVP: geometry not set");
    if (!tmask || !umaskCD || !emask || !nmask || !fcor_blk || !fcorE_blk || !fcorN_blk) return fail(-1, "null argument");
    // Where the blocks next to the fold have several owners the T-grid fields go through the fold exchange and the centre fold
    // step of its lists (cice_evp_hip_cgrid_prep).  What stays refused is a fold neighbourhood with an eliminated block on a
    // layout without that exchange: the rank-local lists cannot name its cells
    if (!fold_exchange() && (S.plan.center_fold_remote || (S.plan.tfold && S.plan.center_tf_remote)))
        return fail(-9, "device preparation: T-grid ghost cells across the tripole fold live on other ranks here; keep "
                        "evp()'s host preparation (cice_evp_hip_cgrid_run) on this configuration");
    CGridState::Prep &Q = CG.prep;
    std::vector<uint8_t> h8(S.n);
    auto B = [&](uint8_t *&p, const int32_t *src) -> int {
        if (!p && CG.mem.alloc(p, S.n)) return -1;
        for (size_t k = 0; k < S.n; ++k) h8[k] = src[k] != 0;
        HIPC(hipMemcpy(p, h8.data(), S.n, hipMemcpyHostToDevice));
        return 0;
    };
    if (B(Q.tmask, tmask) || B(Q.xmask[0], umaskCD) || B(Q.xmask[1], emask) || B(Q.xmask[2], nmask)) return -1;
    const double *fc[3] = {fcor_blk, fcorE_blk, fcorN_blk};
    for (int k = 0; k < 3; ++k)
        if ((!Q.fcor[k] && zeros(Q.fcor[k], S.n)) || h2d(Q.fcor[k], fc[k])) return -1;
    // (with the staging slots of the fold exchange: the ten halo-updated ones travel through it)
    for (auto &p : Q.t)
        if (!p && zeros(p, field_len())) return -1;
    if ((!Q.tmass && zeros(Q.tmass, field_len())) || (!Q.maskd && zeros(Q.maskd, field_len()))) return -1;
    const HaloPlan &P = S.plan;
    Q.n_center = (int)P.center_dst.size();
    if (Q.n_center && !Q.c_dst) {
        if (CG.mem.upload(Q.c_dst, P.center_dst) || CG.mem.upload(Q.c_src, P.center_src) || CG.mem.upload(Q.c_vsign, P.center_vsign)) return -1;
    }
    // the loop's inputs persist between calls as the reference's module arrays do (a cell off the ice keeps e.g. its fmE)
    for (auto &p : CG.in) HIPC(hipMemsetAsync(p, 0, S.n * sizeof(double), S.stream));
    HIPC(hipMemsetAsync(CG.mask4, 0, 4 * S.n * sizeof(int32_t), S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    Q.geo = true;
    return 0;
}

static void fill_prep(EvpCgPrep &P)
{
    CGridState::Prep &Q = CG.prep;
    P.nx = S.d.nx_block; P.ny = S.d.ny_block; P.plane = S.plane; P.n = S.n; P.blk = S.blk;
    for (int k = 0; k < 11; ++k) P.t[k] = Q.t[k];
    P.tmass = Q.tmass; P.maskd = Q.maskd;
    P.hm = CG.g[CG_HM]; P.tarea = CG.g[CG_TAREA]; P.uarea = CG.g[CG_UAREA]; P.earea = CG.g[CG_EAREA]; P.narea = CG.g[CG_NAREA];
    for (int k = 0; k < 3; ++k) { P.xmask[k] = Q.xmask[k]; P.fcor[k] = Q.fcor[k]; }
    P.m4 = CG.mask4;
    for (int k = 0; k < 14; ++k) P.f[k] = CG.f[k];
    for (int k = 0; k < CG_NIN; ++k) P.in[k] = CG.in[k];
    P.dt = Q.pp.dt; P.gravit = Q.pp.gravit; P.dyn_area_min = Q.pp.dyn_area_min; P.dyn_mass_min = Q.pp.dyn_mass_min;
    P.cosw = S.prm.cosw; P.sinw = S.prm.sinw; P.ssh_coupled = Q.pp.ssh_stress_coupled;
}

int cice_evp_hip_cgrid_prep(const cice_evp_hip_prep_params *pp, const double *const *tfields11,
                            const double *const *state12, int32_t *iceTmask, int32_t *iceUmask, int32_t *iceEmask,
                            int32_t *iceNmask)
{
    if (!S.ready || !CG.geo) return fail(-1, "C-grid EVP: geometry not set");
    CGridState::Prep &Q = CG.prep;
    if (!Q.geo) return fail(-1, "cice_evp_hip_cgrid_set_prep_geometry was not called");
    if (!pp || !tfields11 || !iceTmask || !iceUmask || !iceEmask || !iceNmask) return fail(-1, "null argument");
    if (int rc = check_tfields(tfields11)) return rc;
    EvpCgPrep P{};
    {   // the forcing layout (cice_evp_hip_set_forcing_layout), checked before anything moves
        const double *area[4] = {CG.g[CG_TAREA], CG.g[CG_UAREA], CG.g[CG_EAREA], CG.g[CG_NAREA]};
        const double *pm[4] = {CG.g[CG_HM], CG.g[CG_UVM], CG.g[CG_EPM], CG.g[CG_NPM]};
        if (int rc = forcing_of(P.F, area, pm)) return rc;
#ifdef CICE_EVP_HIP_TESTING
        if (P.F.on)
            for (int k = 0; k < 4; ++k) {
                if (!Q.prod[k] && zeros(Q.prod[k], S.n)) return -1;
                P.F.prod[k] = Q.prod[k];
            }
#endif
    }
    // the loop's state: given, or NULL = what the previous call left on the device (evp() is its only writer)
    int nstate = 0;
    if (state12)
        for (int k = 0; k < 12; ++k) nstate += state12[k] != nullptr;
    if (nstate != 0 && nstate != 12) return fail(-1, "state arrays: give all 12 or none");
    if (nstate == 0 && !CG.uploaded) return fail(-1, "no C-grid state on the device yet: the first call must upload it");
    Q.pp = *pp;
    HIPC(hipEventRecord(S.ev2, S.stream));
    CopyBatch B;
    for (int k = 0; k < 11; ++k) B.items.push_back({Q.t[k], tfields11[k]});
    if (nstate)
        for (int k = 0; k < 12; ++k) B.items.push_back({CG.f[k], state12[k]});
    if (h2d_batch(B)) return -1;
    {   // the previous call's ice masks at U, E, N points (ghost cells included: they travel back unchanged)
        const int32_t *m[3] = {iceUmask, iceEmask, iceNmask};
        for (int k = 0; k < 3; ++k)
            HIPC(hipMemcpyAsync(CG.mask4 + (size_t)(k + 1) * S.n, m[k], S.n * sizeof(int32_t), hipMemcpyHostToDevice, S.stream));
    }
    HIPC(hipEventRecord(S.ev3, S.stream));
    {   // dyn_prep1 and the T-grid halo updates: the B-grid preparation's kernels
        EvpPrep P{};
        P.nx = S.d.nx_block; P.ny = S.d.ny_block; P.plane = S.plane; P.blk = S.blk;
        P.tmask = Q.tmask;
        for (int k = 0; k < 11; ++k) P.t[k] = Q.t[k];
        P.tmass = Q.tmass; P.maskd = Q.maskd;
        P.rhoi = pp->rhoi; P.rhos = pp->rhos; P.dyn_area_min = pp->dyn_area_min; P.dyn_mass_min = pp->dyn_mass_min;
        evp_launch_prep1(P, S.d.nblocks, S.stream);
        EvpPrepHalo H{};
        std::pair<double *, bool> arrs[10] = {{Q.maskd, false}, {Q.tmass, false}, {Q.t[3], false}, {Q.t[4], false}, {Q.t[5], true},
                                              {Q.t[6], true}, {Q.t[7], true}, {Q.t[8], true}, {Q.t[9], true}, {Q.t[10], true}};
        // calc_strair = .false.: strax / stray in slots 9 / 10 are averaged as the host holds them (ice_dyn_evp.F90:467-468)
        const int nh = S.forcing.wind_t() ? 10 : 8;
        for (int k = 0; k < nh; ++k) { H.a[H.narr] = arrs[k].first; H.is_vec[H.narr] = arrs[k].second; ++H.narr; }
        H.dst = Q.c_dst; H.src = Q.c_src; H.vsign = Q.c_vsign; H.n = Q.n_center;
        evp_launch_halo_center(H, S.stream);
        if (fold_exchange()) {
            // the blocks next to the fold on several ranks: pair by pair through the fold exchange (ghost cells other ranks own
            // up to the fold, raw fold sources into the staging slots), then the fold step of location 0 on all of them in one
            // pass -- instead of the list's fold-crossing entries, the T-fold step below and the plain exchange.  Collective:
            // ranks without fold rows take part with empty fold lists.
            double *pairs[5][2] = {{Q.maskd, Q.tmass}, {Q.t[3], Q.t[4]}, {Q.t[5], Q.t[6]}, {Q.t[7], Q.t[8]}, {Q.t[9], Q.t[10]}};
            for (int q = 0; q < nh / 2; ++q)
                if (int rc = cgrid_fold_exchange(pairs[q][0], pairs[q][1], field_len())) return rc;
            double *x[10];
            bool vec[10];
            for (int k = 0; k < nh; ++k) { x[k] = arrs[k].first; vec[k] = arrs[k].second; }
            if (int rc = fold_center_batch(x, vec, nh, field_len())) return rc;
        } else if (CG.tfold) {
            // tripoleT: the centre rule rewrites the top physical row (made symmetric, then mirrored) and fills the ghost row
            // from row NY-1: the fold step of location 0, after the plain ghost copies (whose sources it does not write)
            fold({{arrs[0].first, 0, arrs[0].second}, {arrs[1].first, 0, arrs[1].second}, {arrs[2].first, 0, arrs[2].second}, {arrs[3].first, 0, arrs[3].second}});
            fold({{arrs[4].first, 0, arrs[4].second}, {arrs[5].first, 0, arrs[5].second}, {arrs[6].first, 0, arrs[6].second}, {arrs[7].first, 0, arrs[7].second}});
            if (nh == 10) fold({{arrs[8].first, 0, arrs[8].second}, {arrs[9].first, 0, arrs[9].second}});
        }
        if (S.plan.center_remote && !fold_exchange()) {
            double *pairs[5][2] = {{Q.maskd, Q.tmass}, {Q.t[3], Q.t[4]}, {Q.t[5], Q.t[6]}, {Q.t[7], Q.t[8]}, {Q.t[9], Q.t[10]}};
            for (int q = 0; q < nh / 2; ++q)
                if (int rc = halo_remote_pair(pairs[q][0], pairs[q][1])) return rc;
        }
    }
    fill_prep(P);                              // (P.F: set above)
    evp_launch_cgrid_prep(P, S.d.nblocks, S.stream);
    EvpCgrid A;
    fill(A);
    evp_launch_cgrid_mask(A, CG.mask4, S.stream);
    // ice_dyn_evp.F90:703-731: exchange uvelE, vvelN; the other component at each face and the corner velocities; exchange
    // them -- the tail of a subcycle (phase 4), on every cell (nothing is masked yet)
    evp_launch_cgrid_phase(A, 9, CF_UE, S.stream);
    evp_launch_cgrid_phase(A, 9, CF_VN, S.stream);
    // (never masked: the halo mask is built from this call's iceTmask)
    if (int rc = exchange(A.f[CF_UE], A.f[CF_VN], false)) return rc;
    fold({{A.f[CF_UE], 2, true}, {A.f[CF_VN], 3, true}});
    evp_launch_cgrid_phase(A, 6, 1, S.stream);
    evp_launch_cgrid_phase(A, 4, 1, S.stream);
    if (int rc = exchange(A.f[CF_UN], A.f[CF_VE], false)) return rc;
    if (int rc = exchange(A.f[CF_UU], A.f[CF_VU], false)) return rc;
    fold({{A.f[CF_UN], 3, true}, {A.f[CF_VE], 2, true}, {A.f[CF_UU], 1, true}, {A.f[CF_VU], 1, true}});
    HIPC(hipEventRecord(S.ev1, S.stream));
    Q.h4.resize(4 * S.n);
    HIPC(hipMemcpyAsync(Q.h4.data(), CG.mask4, 4 * S.n * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(S.stream));
    if (fold_exchange())                        // a fold exchange whose wait gave up: nothing goes back to the caller
        if (int rc = direct_check_error()) return rc;
    int32_t *out[4] = {iceTmask, iceUmask, iceEmask, iceNmask};
    for (int k = 0; k < 4; ++k) std::memcpy(out[k], Q.h4.data() + (size_t)k * S.n, S.n * sizeof(int32_t));
    float ms = 0;
    if (hipEventElapsedTime(&ms, S.ev3, S.ev1) == hipSuccess) Q.t_ms = ms;
    Q.pending = true;
    return 0;
}

// seabed stress factors TbE / TbN on the device, LKD method (seabed_stress_factor_LKD with grid_location = 'E' / 'N',
// ice_dyn_shared.F90:1386-1460; call site ice_dyn_evp.F90:803-815), from the aice / vice of the last
// cice_evp_hip_cgrid_prep (ghost cells as given) and the masks it produced.  Between _cgrid_prep and _cgrid_prep_finish.  One device exp() per
// ice face: <= 1 ulp from the host libm's.
int cice_evp_hip_cgrid_seabed_lkd(const double *hwater, double k1, double k2, double alphab, double threshold_hw)
{
    CGridState::Prep &Q = CG.prep;
    if (!Q.pending) return fail(-1, "no prepared C-grid state (cice_evp_hip_cgrid_prep first)");
    if (!Q.hwater) {
        if (!hwater) return fail(-1, "hwater needed on the first call");
        if (zeros(Q.hwater, S.n)) return -1;
    }
    if (hwater && h2d(Q.hwater, hwater)) return -1;
    // aice, vice, hwater are read at (i+1, j) / (i, j+1) as the caller handed them over, ghost cells included -- the
    // reference reads its module arrays the same way (their ghost cells are current in the host model)
    EvpCgPrep P{};
    fill_prep(P);
    evp_launch_cgrid_seabed_lkd(P, S.d.nblocks, CG.mask, Q.hwater, k1, k2, alphab, threshold_hw, S.stream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

// ... probabilistic method (seabed_stress_factor_prob with TbE / TbN, ice_dyn_shared.F90:1475-1683; call site
// ice_dyn_evp.F90:816-827): the T-point factor as on the B grid, then the maximum over the two T-cells of every ice face
int cice_evp_hip_cgrid_seabed_prob(const double *hwater, const double *aicen, const double *vicen, int32_t ncat, double alphab,
                                   double rhoi, double gravit, double pi, double puny)
{
    CGridState::Prep &Q = CG.prep;
    if (!Q.pending) return fail(-1, "no prepared C-grid state (cice_evp_hip_cgrid_prep first)");
    if (!aicen || !vicen || ncat < 1) return fail(-1, "bad argument");
    if (!Q.hwater) {
        if (!hwater) return fail(-1, "hwater needed on the first call");
        if (zeros(Q.hwater, S.n)) return -1;
    }
    if (hwater && h2d(Q.hwater, hwater)) return -1;
    if (Q.ncat != ncat) {
        CG.mem.free_one(Q.aicen);
        CG.mem.free_one(Q.vicen);
        if (zeros(Q.aicen, S.n * (size_t)ncat) || zeros(Q.vicen, S.n * (size_t)ncat)) return -1;
        Q.ncat = ncat;
    }
    if (!Q.tbt && zeros(Q.tbt, S.n)) return -1;
    HIPC(hipMemcpyAsync(Q.aicen, aicen, S.n * (size_t)ncat * sizeof(double), hipMemcpyHostToDevice, S.stream));
    HIPC(hipMemcpyAsync(Q.vicen, vicen, S.n * (size_t)ncat * sizeof(double), hipMemcpyHostToDevice, S.stream));
    EvpPrep PB{};
    PB.nx = S.d.nx_block; PB.ny = S.d.ny_block; PB.plane = S.plane; PB.blk = S.blk;
    PB.mask = CG.mask;                         // bit0 = iceTmask in both layouts
    evp_launch_seabed_prob_t(PB, S.d.nblocks, Q.hwater, Q.aicen, Q.vicen, ncat, alphab, rhoi, S.prm.rhow, gravit, pi, puny, Q.tbt,
                             S.stream);
    EvpCgPrep P{};
    fill_prep(P);
    evp_launch_cgrid_seabed_prob_faces(P, S.d.nblocks, CG.mask, Q.tbt, S.stream);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

// ... or computed by the host after the preparation (the reference's own routines, libm exp(): what the Fortran entry does)
int cice_evp_hip_cgrid_set_tb(const double *TbE, const double *TbN)
{
    if (!CG.prep.pending) return fail(-1, "no prepared C-grid state (cice_evp_hip_cgrid_prep first)");
    if (!TbE || !TbN) return fail(-1, "null argument");
    if (h2d(CG.in[CI_TBE], TbE) || h2d(CG.in[CI_TBN], TbN)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

// ice strength (the host's: icepack_ice_strength + its halo update, ice_dyn_evp.F90:596-608, 727-728) and the per-call
// set-up of the loop; cice_evp_hip_cgrid_subcycle / _download follow as after cice_evp_hip_cgrid_upload
int cice_evp_hip_cgrid_prep_finish(const double *strength, int32_t visc_method)
{
    CGridState::Prep &Q = CG.prep;
    if (!Q.pending) return fail(-1, "no prepared C-grid state (cice_evp_hip_cgrid_prep first)");
    if (!strength) return fail(-1, "null argument");
    if (visc_method != 0 && visc_method != 1) return fail(-1, "visc_method %d (0 avg_zeta, 1 avg_strength)", visc_method);
    if (h2d(CG.in[CI_STRENGTH], strength)) return -1;
    Q.pending = false;
    return finish_upload(visc_method);
}

// what the preparation left on the device, for hosts that need it (dyn_finish at E / N points reads aiX, fmX, uocnX,
// vocnX) and for the tests: table 0 = the loop's 19 state / work arrays, 1 = its 23 inputs
int cice_evp_hip_cgrid_fetch(int32_t table, int32_t index, double *dst)
{
    if (!S.ready || !CG.geo) return fail(-1, "C-grid EVP: geometry not set");
    if (!dst) return fail(-1, "null argument");
    const double *src = nullptr;
    if (table == 0 && index >= 0 && index < CG_NF) src = CG.f[index];
    if (table == 1 && index >= 0 && index < CG_NIN) src = CG.in[index];
#ifdef CICE_EVP_HIP_TESTING
    // the test build: what the last preparation with a forcing layout averaged -- strairxE strairyN ss_tltxE ss_tltyN
    if (table == 2 && index >= 0 && index < 4) src = CG.prep.prod[index];
#endif
    if (!src) return fail(-1, "cgrid_fetch: table %d index %d", (int)table, (int)index);
    if (d2h(dst, src)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

#ifdef CICE_EVP_HIP_TESTING
// Phase stamps of the last cg_one launch (CICE_EVP_HIP_CGRID_PROF=1 at cice_evp_hip_cgrid_set_geometry): [windows][8] x u64.
// Returns the number of windows, < 0 on error.
int cice_evp_hip_debug_cgres_prof(uint64_t *out, int32_t ntiles_max)
{
    if (!S.ready || !CG.res.prof) return fail(-1, "no profiled resident C-grid launch (CICE_EVP_HIP_CGRID_PROF=1)");
    if (!out || ntiles_max < CG.res.ntiles) return fail(-1, "bad argument: need room for %d windows", CG.res.ntiles);
    HIPC(hipStreamSynchronize(S.stream));
    HIPC(hipMemcpy(out, CG.res.prof, (size_t)CG.res.ntiles * 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return CG.res.ntiles;
}

int cice_evp_hip_debug_cgrid_prof(uint64_t *out, int32_t ntiles_max)
{
    if (!S.ready || !CG.one.prof) return fail(-1, "no profiled one-launch kernel (CICE_EVP_HIP_CGRID_PROF=1)");
    if (!out || ntiles_max < CG.one.ntiles) return fail(-1, "bad argument: need room for %d windows", CG.one.ntiles);
    HIPC(hipStreamSynchronize(S.stream));
    HIPC(hipMemcpy(out, CG.one.prof, (size_t)CG.one.ntiles * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return CG.one.ntiles;
}

// The shortcut verdicts of the call about to run, see the testing header: B-grid word, C-grid word, CG.fast
int cice_evp_hip_debug_call_flags(uint32_t *out, int32_t n)
{
    if (!S.ready) return fail(-1, "not initialised");
    const uint32_t v[4] = {S.flags & S.flags_allowed, CG.uploaded ? g_last_call_flags : 0u, (CG.uploaded && CG.fast) ? 1u : 0u,
                           (S.res_ran && S.res2_lean) ? 1u : 0u};
    int32_t k = 0;
    for (; out && k < n && k < 4; ++k) out[k] = v[k];
    return k;
}
#endif

int cice_evp_hip_cgrid_timings(double *out, int32_t n)
{
    if (!out || n < 2) return fail(-1, "need room for 2 values");
    const int *ran = CG.last.count;              // the last call's subcycles by what ran them
    const MarchItems &Z = CG.one.zone;
    out[0] = CG.t_loop_ms;
    out[1] = (double)CG.t_nsub;
    if (n >= 3) out[2] = CG.prep.t_ms;           // device time of the last cice_evp_hip_cgrid_prep (kernels, without the copies)
    if (n >= 4) out[3] = (double)ran[CG_ONE];    // subcycles of the last call run as one launch each
    if (n >= 5) out[4] = geo_derived() ? 1.0 : 0.0;   // ... with 15 of the 23 static arrays derived in the kernel
    if (n >= 6) out[5] = (double)CG.res.last_nsub;    // subcycles of the last call inside ONE launch of the on-chip resident kernel
    if (n >= 7) out[6] = CG.res.t_probe_ms;           // ... and what its probe measured per subcycle, ms (-1: no probe ran)
    if (n >= 8) out[7] = (double)CG.res.fallbacks;    // cice_evp_hip_cgrid_run calls repeated without it after one of its waits gave up
    if (n >= 9) out[8] = (double)CG.res.n_live;       // windows of the resident kernel that hold ice in this call (only they run) ...
    if (n >= 10) out[9] = (double)CG.res.ntiles;      // ... of so many
    if (n >= 11) out[10] = (double)Z.nitems;          // the one-launch schedule's marched kernel (cg_strip): work items (0: not in use) ...
    if (n >= 12) out[11] = (double)Z.cells;           // ... the cells it owns ...
    if (n >= 13) out[12] = (double)CG.one.ntiles_e;   // ... and the windows cg_one keeps beside it
    if (n >= 14) out[13] = (double)Z.seg;             // ... rows per segment
    if (n >= 15) out[14] = (double)Z.len;             // ... 1: it forms six of the eight lengths from dxN, dyE
    if (n >= 16) out[15] = fold_exchange() ? 1.0 : 0.0;            // tripole: the blocks next to the fold on several ranks (fold exchange)
    if (n >= 17) out[16] = CG.tripole ? (double)S.plan.cg_fold_ranks : 0.0;   // ... on so many ranks
    if (n >= 18) out[17] = fold_exchange() ? (double)S.plan.cg_tail : 0.0;    // ... staging slots of this rank
    if (n >= 20) {
        out[18] = (double)(ran[CG_ZONE_FRAME] + ran[CG_ZONE_FRAME_PHASES]);   // subcycles of the last call that ran as "zone marched + frame" (several ranks)
        out[19] = (double)CG.fr.ncells;               // ... and the frame cells of this rank (0: no such plan here)
        if (ran[CG_ZONE_FRAME_PHASES] > 0) {          // (the five-phase frame plan ran: its frame cells, its own items)
            const MarchItems &M = CG.mf.zone;
            out[19] = (double)CG.mf.frame_cells;
            out[10] = (double)M.nitems; out[11] = (double)M.cells; out[14] = (double)M.len;
        }
    }
    if (n >= 23) {
        out[20] = (double)ran[CG_MARCH_FOLD];         // subcycles of the last call that ran as "marched zone + fold band" (tripole grids, one rank)
        out[21] = (double)CG.mf.band_rows;            // ... rows from the zone's top row to the fold (0: no such plan here)
        out[22] = (double)CG.mf.rest.ncells;               // ... and the cells the five list-driven phase kernels advance
    }
    if (n >= 26) {
        out[23] = (double)ran[CG_MARCH_FOLD_RANKS];   // subcycles of the last call that ran as "marched zone + fold band + frame" (tripole grids, several ranks)
        out[24] = (double)CG.mf.frame_cells;          // ... the frame cells among the rest cells (sent to another rank, or with a ghost image here)
        out[25] = (ran[CG_MARCH_FOLD_RANKS] > 0 && fold_exchange()) ? 1.0 : 0.0;   // ... 1: with the fold exchange (the fold rows on several ranks)
    }
    if (n >= 27) out[26] = (double)CG.in_alt;         // bit q: PP_FIELDS[q] is in its second allocation now (where the last call left it)
    return 0;
}

}  // extern "C"
