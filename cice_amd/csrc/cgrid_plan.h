// Host-side planners of the C grid's kernels, derived from a rank's halo plan (halo_plan.h): the window tables of the one-launch
// and resident kernels, the marched kernel's rectangles and items, the zone / rest split of a rank beside list-driven kernels,
// and the resident kernel's hand-off graph.  Host only, CPU-tested.
#pragma once
#include "halo_plan.h"

// Window table of the C grid's one-launch kernel (evp_cgrid.hip: cg_one; host only).  Windows of ox x oy positions, the
// inner (ox-3) x (oy-3) owned cells, cover every block's interior row by row (in strips of `strip` windows in x).  Per
// window 4 ints in `tiles` -- block, first owned i, first owned j (1-based, array numbering), 1 if the window is regular
// (every position an array cell of that block and its own source) -- and ox*oy entries in `tab`: for the position
// (tx, ty) = cell (i0-2+tx, j0-2+ty) of the block's numbering, which may lie outside its array, the cell whose value the
// reference has there: >= 0 an interior cell (itself, or the one a ghost cell mirrors according to the plan's local
// copies; further out the walk continues from the mirrored cell, neighbour by neighbour, x first), or -1 - c for a ghost
// cell c nothing is copied into (closed boundary, eliminated neighbour block): its arrays are read, never computed.
// extra = 1: (ox+1) x (oy+1) positions per window, same owned range and window stride (the resident kernel's velocity tile).
void build_window_table(const cice_evp_hip_dims &d, const HaloPlan &plan, int ox, int oy, int strip, std::vector<int32_t> &tiles,
                        std::vector<int32_t> &tab, int extra = 0);

// The same for a tripole (u-fold) grid (17 x 17 positions): the top window row of the blocks at the fold carries a mirrored
// mini-tile in source orientation above the fold row; see cgrid_plan.cpp.  tiles2: (G0, NX, 0, 0) per window.
bool build_fold_window_table(const cice_evp_hip_dims &d, const HaloPlan &plan, std::vector<int32_t> &tiles, std::vector<int32_t> &tiles2,
                             std::vector<int32_t> &tab, std::string &why);

// Which positions of a resident window's 17 x 17 velocity tile are hand-offs (evp_cgrid_res.hip polls them, their owner publishes
// them): not owned, with a producing cell, and within reach of the window's owned cells -- at most CGRES_REACH positions beyond
// the last owned column and row (an owned cell's divergence reads level U beside it, that level T one further, that the velocities
// one further again: two; three is the kernel's own margin).  Everything further out is worked out from whatever the tile was filled
// with and read by nobody.  Without the bound a narrow window at a block's edge (one or two owned columns) polled up to 14 columns
// into its neighbour and beyond -- cells of a window that does not poll IT: that window could run two subcycles ahead and overwrite
// the record slot the narrow one was still waiting for (round-5 advice).  Fold windows keep every position (their mirrored mini-tile
// runs against the column index).
constexpr int CGRES_REACH = 3;
constexpr int CGRES_SLOTS = 4;             // record slots per cell, by subcycle modulo (evp_device.h: EVP_CGRES_SLOTS)
inline bool cgres_in_reach(int ex, int ey, int last_ex, int last_ey, bool foldwin)
{
    return foldwin || (ex <= last_ex + CGRES_REACH && ey <= last_ey + CGRES_REACH);
}
// ---- the marched C-grid kernel's share of a rank (evp_cgrid.hip: cg_strip) -- host only, CPU-tested ----
// A rectangle of a block that the regular windows of a window table cover (regular: every position an interior cell of the block,
// its own source): first owned column / row of its first and last window column / row.
struct StripZone { int b, i0, i1, j0, j1; };
// A range of cells of one block's array, 1-based, both ends included.
struct StripRange { int i0, i1, j0, j1; };
// What cg_strip reads for the work item (b, c, ja, jb, lo, hi) -- every load of the kernel, counted from its loop: lanes 0 .. 63 hold
// columns c - 2 .. c + 61 and load unconditionally (lane 63 only loads).  The iterations run j = j0 .. jb + 1, j0 = ja - 4 (LEN:
// ja - 5, one earlier, so that dxE of row ja - 2 finds HTN of row ja - 3); each loads row j + 2 ahead (uE, dxE or HTN, dyE, the
// land and ice masks -- the last iteration's too, which nothing uses), row j + 1 (vN, the other lengths, stresses, strength) and
// row j - 1 (the momentum step's operands).  Rows ja - 5 .. jb + 3 (LEN: ja - 6 .. jb + 3).  The lane-shifted HTN / HTE of LEN are
// register moves between these lanes, no further loads.
inline StripRange strip_footprint(const int32_t *item, bool len)
{
    return StripRange{item[1] - 2, item[1] + 61, item[2] - (len ? 6 : 5), item[3] + 3};
}
// per block the rectangle of its regular windows, if they form one, it is at least a strip wide and none of its cells has a ghost
// image (img_slot: per cell, < 0 = none; may be null).  Window rows come off its top (then its bottom), window columns off its east
// (then its west) side until the footprint of every item strip_items can make of it -- with the lengths formed or loaded -- lies
// inside the block's array: the windows taken off stay with cg_one.
// min_cols: the narrowest rectangle kept (a strip's 62 columns where the windows of cg_one take what is left; the fold-band plan keeps
// any whole window column -- its items then own fewer lanes).
void strip_zones(const cice_evp_hip_dims &d, const std::vector<int32_t> &tiles, int ex, int ey, const int *img_slot, std::vector<StripZone> &zones,
                 int min_cols = 62);
// The cells on which the host checks, bit for bit, that the six lengths cg_strip<LEN> would form equal the loaded ones.  The kernel
// forms dxT, dyT, dxU, dyU, dxE, dyN from HTN and HTE on columns c - 2 .. c + 61 (every lane) and rows ja - 2 .. jb + 2 of an item
// (dxE of row jb + 2 enters the shear of row jb + 1, which the stresses of row jb + 1 and so the owned row jb use); r is the
// rectangle all items of z (lo0 = 3) form lengths on.  False if that reaches a cell whose formula needs a neighbour outside the
// block's array (the outermost row or column): such a rectangle cannot be verified, LEN is refused for it.
bool strip_len_range(const StripZone &z, int ex, int ey, int nx_block, int ny_block, StripRange &r);
// work items of the rectangles, x 6 ints each: block, column of lane 2, first and last owned row, first and last owned lane.  lo0: first lane
// that may own a column (2; 3 where the kernel forms the lengths), the last is 61; strips of 62 - lo0 columns, the last one shifted west
// so that lane 62 stays inside the rectangle + 1; segments of `seg` rows (0: the fewest rows >= seg_min with at most `slots` items).
// Returns the rows per segment.
int strip_items(const std::vector<StripZone> &zones, int ex, int ey, int lo0, long slots, int seg_min, int seg, std::vector<int32_t> &items);
// 1 for every window of `tiles` that lies inside one of the rectangles (the marched kernel owns its cells), 0: cg_one keeps it
void strip_windows(const std::vector<StripZone> &zones, const std::vector<int32_t> &tiles, std::vector<uint8_t> &in_zone);

// The rectangles of a rank from its halo plan: the table of ex x ey windows (tiles, x 4 as above), the map of the cells that have a
// ghost image among the rank's own copies, and strip_zones with both.  last_image_row: a ghost cell in a global row above it is no
// image (build_cg_march_fold: the rows the fold step fills); STRIP_EVERY_IMAGE: every ghost cell with a source is one.
constexpr int STRIP_EVERY_IMAGE = 1 << 30;
void plan_strip_zones(const cice_evp_hip_dims &d, const HaloPlan &P, int ex, int ey, int min_cols, int last_image_row, std::vector<int32_t> &tiles,
                      std::vector<StripZone> &zones);

// ---- the marched kernel beside list-driven kernels: a rank's interior cells split in two ----
// The ZONE -- the cells cg_strip's items own -- and the REST, every other interior cell, which list-driven variants of the un-fused or
// fused kernels advance (evp_cgrid.hip).  Three schedules split a rank this way: several ranks (build_cg_frame; the rest is the FRAME
// around each block's rectangle), a tripole / tripoleT grid on one rank (build_cg_march_fold; the rest is the band under the fold and
// the block edges) and such a grid on several ranks (build_cg_march_fold again; the rest holds band and frame).  A rest cell reads intermediates of its neighbours, so each level also runs on the zone cells the next level reads
// ("dilation"; a zone cell evaluated for a rest cell's sake stores to scratch arrays only).  Each plan is a table of reads -- level, the
// level that produces what it reads, offsets, in cgrid_plan.cpp -- which one helper walks to mark the cells of every level and walks
// again to check them.  Level T (stressC_T) also runs on the reference's extra T row and column (ghost cells i = ihi + 1, j = jhi + 1,
// which keep stress12T only); no other level runs on a ghost cell.
// cells: per array cell the EVP_CGS_* bits (evp_device.h); wg[k]: the workgroups of 64 x 4 cells ((b * gy + by) * gx + bx, gx =
// ceil(nx_block / 64), gy = ceil(ny_block / 4)) that hold a cell of the plan's k-th level, ascending.
// Both planners return 1 and the plan; 0 with `why` where the schedule does not apply; -1 with `why` when an invariant of the plan does
// not hold: the two sets are disjoint and cover the interior; a rest cell runs every level itself; every value a level reads at an
// interior cell is produced by the level before it (or is the previous subcycle's); level T's loads, and the stencil of every other
// evaluated cell (one cell around it), lie inside the block's array.
struct CgSplitPlan {
    std::vector<uint8_t> cells;
    std::vector<int32_t> wg[5];
    long zone_cells = 0, rest_cells = 0;
};

// ---- several ranks (evp_host_cgrid.cpp: "zone marched + frame"): the frame variants of the three fused kernels, cg_frame_* ----
//   level C (momentum step; EVP_CGS_REST) on the frame cells; it reads etax2T around its three corners and the new stresspT / stressmT of
//           its east and north neighbour (T cells within one of it), and shearU at its own, south and west corner;
//   level T (stressC_T) on those T cells; it reads shearU at its four corners (own, west, south, south-west);
//   level S (strain_rates_U's shear) on every interior cell one of the two reads shearU of.
// wg[0 .. 2]: levels S, T, C.  items: x 6 as strip_items makes them (may be empty: every interior cell is a frame cell).  Declines (0)
// when the rank has no neighbour on another rank: the one-launch schedule serves it.  Its own invariant: every cell a peer receives and
// every cell with a ghost image on this rank is a frame cell.
using CgFramePlan = CgSplitPlan;
int build_cg_frame(const cice_evp_hip_dims &d, const HaloPlan &P, const std::vector<int32_t> &items, CgFramePlan &F, std::string &why);

// ---- a tripole / tripoleT grid on one rank (evp_host_cgrid.cpp: "marched zone + fold band") or on several ("... + frame"): the five
// un-fused phase kernels, cg_band_*, with the fold steps -- and across ranks the exchanges -- of the five-phase schedule ----
// The zone: strip_zones' rectangles, cut from the top in the blocks at the fold until the fold rule holds for every item.  The fold rule
// (what cg_strip forms, by field location and row, counted from its loop; jb = an item's last owned row):
//   * nothing is FORMED at a point on the fold or beyond it.  The kernel forms, up to row jb + 1, the face -> corner and face <-> face
//     averages of the previous subcycle's velocities (corner, N face, E face), the shear at the corner and stressC_T at the centre; up
//     to row jb deltaU, etax2U and stress12U (corner) and the momentum step (E and N face): strip_form_top.  On the fold lie row NY of
//     the N-face and NE-corner locations (u-fold), row NY of every location (T-fold); beyond it the ghost row NY + 1.
//   * everything LOADED (strip_footprint) lies inside the block's array; of the arrays the loop writes, rows NY and NY + 1 hold what the
//     fold step of the previous subcycle left there: no fold-list source or destination may be a zone cell, so the fold step of a
//     subcycle finds every operand written by the REST's kernels on its own stream.
//   * the static arrays the kernel derives must be the caller's on every cell an item derives them for: `geo` (below).
// The levels:
//   phase 3 (div_stress + stepu_C / stepv_C; EVP_CGS_REST) on the REST cells; it reads stress12U at its own, south and west corner, the new
//           stresspT / stressmT at its own cell and the east / north neighbour;
//   phase 2 (etax2U, stressC_U; EVP_CGS_U) on those corners; it reads etax2T at the four T cells around the corner and the corner's shearU;
//   phase 1 (stressC_T; EVP_CGS_T) on those T cells; it reads shearU at its four corners;
//   phase 0 (strain_rates_U; EVP_CGS_S) on those corners; it reads uvelN / vvelE at the cell, its east / north neighbour, uvelU / vvelU at
//           the cell;
//   phase 4 (the averages, AFTER the two sets have met again; EVP_CGS_AVG) on the REST cells and on every cell phase 0 of the next subcycle
//           reads (uvelN, vvelE, uvelU, vvelU are not the marched kernel's: phase 4 stores to the arrays themselves on zone cells too).
// wg[0 .. 4]: phases 0 .. 4.  EVP_CGS_FOLDROW marks the interior cells of global row NY.
// last row, relative to an item's last owned row, at which cg_strip forms a value of field location loc (0 centre, 1 NE corner, 2 E
// face, 3 N face) -- from the kernel's loop: it runs to j = jb + 1 and evaluates levels S and T and both face averages (the N-face one
// in the last subcycle of a call) on row j, levels U and C on row j - 1
constexpr int STRIP_AHEAD = 1;             // == EVP_CGSTRIP_AHEAD (evp_device.h): the loop's last iteration is j = jb + STRIP_AHEAD
struct StripLevel { const char *what; int loc, first, last; };      // rows first .. last, relative to (ja, jb), of location loc
constexpr StripLevel STRIP_LEVELS[] = {
    {"face -> corner averages of the previous subcycle", 1, -2, STRIP_AHEAD},
    {"E -> N average (the last subcycle of a call: one row more)", 3, 0, STRIP_AHEAD},
    {"N -> E average", 2, 0, STRIP_AHEAD},
    {"shearU", 1, -2, STRIP_AHEAD},
    {"deltaU", 1, 0, 0},
    {"stressC_T", 0, -2, STRIP_AHEAD},
    {"etax2U, stress12U", 1, -1, 0},
    {"momentum step, E face", 2, 0, 0},
    {"momentum step, N face", 3, 0, 0},
};
inline int strip_form_top(int loc)
{
    int top = -(1 << 30);
    for (const StripLevel &l : STRIP_LEVELS)
        if (l.loc == loc) top = top > l.last ? top : l.last;
    return top;
}
struct CgMarchFoldPlan : CgSplitPlan {
    std::vector<int32_t> items;            // x 6, as strip_items makes them
    std::vector<StripZone> zones;
    int band_rows = 0;                     // rows from the zone's top row (exclusive) to NY, on the blocks at the fold (the most)
    int seg = 0, lengths = 0;              // rows per segment; 1: the items own lanes >= 3 (the kernel forms six of the eight lengths)
    std::vector<int32_t> sent;             // several ranks: the interior cells another rank receives in an in-loop exchange, ascending
    long frame_cells = 0;                  // REST cells that are sent or have a ghost image on this rank (the FRAME)
};
// geo (may be null: everything holds): what the caller's static arrays allow for the rectangle z -- 0 an identity fails on a cell the
// kernel would derive it for (a window row comes off the top and the question is asked again), 1 the 15 derived arrays hold, 3 the six
// formed lengths hold as well.  The items own lanes >= 3 (lengths = 1) when every rectangle answers 3 and want_len != 0.
// Declines (0) without a fold and when no rectangle is left under the band.  Its own invariants: every fold-list source and destination
// that is an interior cell is a REST cell, evaluated at its level (an operand >= the rank's cells is a staging slot and needs none); no
// item forms a value on the fold.
// Several ranks ("marched zone + fold band + frame"; allow_ranks = false declines them, the one-rank question): the same plan on any
// rank layout the five phases take.  The fold lists are the host's -- HaloPlan::cg_fold where the fold rows have several owners,
// build_fold_list's where they are all here, none on a rank without them (zone + frame, band_rows = 0) -- and the REST also holds the
// FRAME: every cell a peer receives (HaloPlan::peers and cg_peers send lists, the raw fold sources for other ranks' staging slots
// included) and every cell with a ghost image here.  One more invariant: each of those is a REST cell evaluated at every level.
// A grid WITHOUT a fold on several ranks (allow_ranks; evp_host_cgrid.cpp: "zone marched + frame" on the five phases, the schedule of
// visc_method = avg_strength there): the same plan with no fold cells and no rows cut from the top -- the REST is the frame as
// build_cg_frame defines it and what strip_zones leaves along the block edges; band_rows = 0.  On one rank, or with allow_ranks =
// false, such a grid declines.
// visc_method = avg_strength changes nothing in a plan: cg_strip<AVGS> loads the same rows (strip_footprint), and what it forms beyond
// the avg_zeta instantiations -- both face averages on rows ja - 1 and jb + 1, deltaU on rows ja - 1 .. jb -- stays within
// STRIP_LEVELS' last rows (LAST forms the same on row jb + 1) and one row below the first owned one, where shearU is formed anyway;
// phase 2 of the list-driven kernels then reads deltaU of its own corner (phase 0 runs wherever phase 2 does) and no etax2T.
struct CgGeoCheck {
    virtual int operator()(const StripZone &z) const = 0;
    virtual ~CgGeoCheck() {}
};
int build_cg_march_fold(const cice_evp_hip_dims &d, const HaloPlan &P, int ex, int ey, long slots, int seg_min, int seg, int want_len,
                        const CgGeoCheck *geo, CgMarchFoldPlan &F, std::string &why, bool allow_ranks = true);

// The hand-off graph of the resident windows (tiles / tab as build_window_table(..., 16, 16, ., extra = 1) or
// build_fold_window_table made them): window w READS window p when it polls a cell p owns.  A window cannot start subcycle j + 1
// before every window it reads has finished subcycle j, so a window p is never more than len subcycles ahead of w, len = the
// shortest chain p reads ... reads w.  The exact-tag record protocol with CGRES_SLOTS slots per cell is safe for the hand-off
// w reads p iff that chain is at most CGRES_SLOTS - 1 long (p's record of subcycle j is overwritten by that of j + CGRES_SLOTS):
// 1 when the hand-off is mutual -- nearly all are --, 2 or 3 for the one-way ones of narrow windows and of fold windows whose
// mirror images do not line up.  pub (may be NULL): [ncell] 1 = the cell is polled by some window, i.e. its owner publishes it.
// Returns the number of UNSAFE hand-offs (no chain back within CGRES_SLOTS - 1); *n_edges, *n_oneway (may be NULL): hand-offs in
// all, and those that are not mutual.
int cgres_dependencies(const cice_evp_hip_dims &d, bool tripole, const std::vector<int32_t> &tiles, const std::vector<int32_t> &tab,
                       std::vector<uint8_t> *pub, int *n_edges, int *n_oneway);
