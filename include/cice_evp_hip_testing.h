/* =====================================================================
 * cice_evp_hip_testing.h -- entry points of the TEST build only.
 *
 * libcice_evp_hip_testing.so = the sources of libcice_evp_hip.so compiled with -DCICE_EVP_HIP_TESTING: the same
 * kernels and host code, plus what tests and tools need and a production host must never find by accident:
 *   - host-only introspection of the halo / seam / marching / window plans (CPU known-answer tests),
 *   - read-outs of the resident kernel's per-CU placement record and phase stamps (tools/),
 *   - a test transport that routes the marching path's exchanges through host callbacks (several ranks as
 *     processes sharing ONE GPU, where RCCL refuses to run),
 *   - the experiment / fault-injection environment switches (evp_host.h: env_test) -- in the production build they
 *     read as unset.
 * The production ABI is include/cice_evp_hip.h.
 * ===================================================================== */
#ifndef CICE_EVP_HIP_TESTING_H
#define CICE_EVP_HIP_TESTING_H

#include "cice_evp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only (no device needed): the fold step of field location `loc` (0 centre, 1 NE corner, 2 E face, 3 N face) on a
 * tripole grid -- x[dst] = s*0.5*(x[a] + isign*x[b]) (b >= 0; -2: partner eliminated) or s*x[a] (b == -1), s = flip ? isign : 1.
 * First call with NULL lists for the count.                                                                       */
int cice_evp_hip_cgrid_fold_plan(const cice_evp_hip_dims *dims, int32_t loc, int32_t *count, int32_t *dst, int32_t *a,
                                 int32_t *b, int32_t *flip);
/* Host only (no device needed): the window table of the C grid's one-launch kernel for windows of ox x oy positions --
 * per window {block, first owned i, first owned j (1-based), regular} in tiles4 and ox*oy entries in tab: the cell whose
 * value the reference has at that position (>= 0), or -1 - c for a ghost cell c nothing is copied into.  First call with
 * NULL arrays for the count.  (What the device kernel reads; checked on the CPU against the decomposition's global numbering.) */
int cice_evp_hip_cgrid_window_plan(const cice_evp_hip_dims *dims, int32_t ox, int32_t oy, int32_t *ntiles, int32_t *tiles4, int32_t *tab);
/* The same with (ox + extra) x (oy + extra) positions per window, extra = 0 or 1 (same owned range and window stride): the table of the
 * on-chip resident C-grid kernel, whose level S reads one position beyond the window to the east and north (evp_cgrid_res.hip).
 * extra = 2: that kernel's table on a tripole (u-fold) grid, 17 x 17 positions (ox, oy unused): the windows at the fold own up to
 * 11 rows and carry a mirrored mini-tile above the fold row, tiles4[3] = fold flag | tf << 8 | last owned row << 16 (cgrid_plan.cpp:
 * build_fold_window_table); -5 when a mirrored cell is not on this rank.                                                          */
int cice_evp_hip_cgrid_window_plan_ext(const cice_evp_hip_dims *dims, int32_t ox, int32_t oy, int32_t extra, int32_t *ntiles,
                                       int32_t *tiles4, int32_t *tab);
/* Host only: the hand-off graph of the on-chip resident C-grid kernel's windows (closed / cyclic grids: the table of extra = 1;
 * tripole: of extra = 2).  A window depends on another when it polls a cell that one owns -- every non-owned position with a
 * producer within 3 positions of its last owned column / row (cgrid_plan.h: cgres_in_reach; fold windows: every position).  n_edges:
 * dependencies, n_oneway: those that are not mutual, n_unsafe: those of them with no chain of at most 3 dependencies back (the
 * window read could then be four subcycles ahead of its reader and overwrite one of the kernel's four record slots per cell that
 * the reader still waits for): the library does not use the kernel unless n_unsafe == 0.                                          */
int cice_evp_hip_cgrid_window_deps(const cice_evp_hip_dims *dims, int32_t *n_windows, int32_t *n_edges, int32_t *n_oneway, int32_t *n_unsafe);
/* Host only: how the one-launch C-grid schedule of large domains shares a rank's cells between the marched kernel (cg_strip) and the
 * windowed kernel (cgrid_plan.h: strip_zones, strip_items, strip_windows, on the window table of ex x ey positions).  items6: per work
 * item block, column of lane 2, first and last owned row (1-based), first and last owned lane (lane l holds column items6[1] - 2 + l);
 * tiles4 / in_zone: the windows (block, first owned i, first owned j, regular) and 1 where the marched kernel owns the window's cells.
 * lo0: first lane that may own a column (2, or 3 where the kernel forms the lengths); slots, seg_min, seg as in strip_items.  Pass NULL
 * arrays to learn the counts.                                                                                                        */
int cice_evp_hip_cgrid_strip_plan(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t lo0, int32_t slots, int32_t seg_min, int32_t seg,
                                  int32_t *n_items, int32_t *items6, int32_t items_cap, int32_t *n_windows, int32_t *tiles4, uint8_t *in_zone, int32_t windows_cap,
                                  int32_t *seg_rows);
/* Host only: the rectangles of cice_evp_hip_cgrid_strip_plan (same dims, ex, ey), 10 ints each in zones10: block, first owned column
 * of its first and last window column, first owned row of its first and last window row (cgrid_plan.h: strip_zones -- window rows and
 * columns already given back where an item would load outside the block's array), 1 if the lengths may be formed for it, and the
 * rectangle of cells the host then checks them on (first and last column, first and last row; cgrid_plan.h: strip_len_range).  The
 * library may still give a window row back where that check fails.  Pass NULL to learn the count.                                    */
int cice_evp_hip_cgrid_strip_zones(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t *n_zones, int32_t *zones10, int32_t zones_cap);
/* Host only: how a rank with neighbours on other ranks shares its interior cells between the marched kernel (the zone: the items of
 * cice_evp_hip_cgrid_strip_plan with the same ex, ey, lo0, slots, seg_min, seg) and the frame variants of the three fused kernels
 * (cice_amd/csrc/cgrid_plan.h: build_cg_frame, which checks the plan's invariants itself and fails with -5 where one does not hold).
 * cells: one byte per array cell -- 1 frame cell, 2 level S (strain_rates_U) runs here, 4 level T (stressC_T), 8 zone cell.  wg: the
 * workgroups of 64 x 4 cells, id = (block * ceil(ny_block / 4) + row) * ceil(nx_block / 64) + column, of level S, then T, then C (the
 * momentum step: frame cells only).  info6 = {zone cells, frame cells, workgroups of S, T, C, items}.  Arrays may be NULL.  Returns
 * 0, or 1 when the rank has no neighbour on another rank (the plan declines: nothing is written but zeros to info6).             */
int cice_evp_hip_cgrid_frame_plan(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t lo0, int32_t slots, int32_t seg_min, int32_t seg,
                                  int64_t *info6, uint8_t *cells, int32_t *wg, int32_t wg_cap, int32_t *items6, int32_t items_cap);
/* Host only: how ONE rank shares the interior of a tripole / tripoleT grid between the marched kernel (the zone: strip_zones' rectangles
 * cut from the top until the fold rule holds) and the list-driven variants of the five phase kernels (the rest: the band under the fold
 * and the block edges) -- cice_amd/csrc/cgrid_plan.h: build_cg_march_fold, which checks the plan's invariants itself (-5 where one fails).
 * len: 1 the items own lanes >= 3 (the kernel forms six lengths), 0 lanes >= 2; slots, seg_min (0: by size), seg as in strip_items.
 * cells: one byte per array cell -- 1 rest cell (phase 3 runs here), 2 phase 0, 4 phase 1, 8 zone cell, 16 phase 2, 32 phase 4, 64 an
 * interior cell of global row NY.  wg: the workgroups of 64 x 4 cells of phases 0 .. 4, numbered as for cice_evp_hip_cgrid_frame_plan.
 * info11 = {zone cells, rest cells, workgroups of phases 0 .. 4, items, fold band rows, rows per segment, len}.  Arrays may be NULL.
 * Returns 0, or 1 when the schedule does not apply -- no fold, several ranks, a grid too short for a zone under the band -- with the
 * reason as the last error's text.
 * ranks: 0 the one-rank question ("marched zone + fold band": several ranks decline); 1 the plan of the rank `dims` describes on any
 * rank layout ("marched zone + fold band + frame"): the rest then also holds every cell another rank receives in an in-loop exchange
 * and every cell with a ghost image; a rank without the fold rows plans zone + frame (0 fold band rows).  ranks3 = {sent cells, frame
 * cells -- sent or with a ghost image --, staging slots behind the arrays}; sent: the sent cells' offsets, ascending.  May be NULL.
 * ranks = 1 on a rank of a grid WITHOUT a fold that has a neighbour on another rank: the plan of "zone marched + frame" with the five
 * list-driven phase kernels on the frame (visc_method = avg_strength there): no fold cells, no rows cut from the top, 0 fold band rows.
 * On one rank, or with ranks = 0, such a grid declines ("no tripole fold ...").  */
int cice_evp_hip_cgrid_march_fold_plan(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t slots, int32_t seg_min, int32_t seg, int32_t len,
                                       int64_t *info11, uint8_t *cells, int32_t *wg, int32_t wg_cap, int32_t *items6, int32_t items_cap,
                                       int32_t ranks, int64_t *ranks3, int32_t *sent, int32_t sent_cap);
/* Test hook: route the exchanges and the rank agreements of the marching path through HOST buffers and the caller's
 * callbacks instead of RCCL (which refuses two ranks on one device), so that its several-rank form can be run as
 * processes sharing one GPU (tools/mailbox_2proc.py --march: torch.distributed gloo underneath).  xchg: per peer q
 * (ascending rank) send_count[q] doubles starting at send + sum of the counts before, likewise recv; returns 0.  reduce:
 * op 0 = min of one int32, 1 = max of one uint32, in place.  NULL callbacks switch the hook off.  Not for production.  */
typedef int (*cice_evp_hip_test_xchg_fn)(void *user, int32_t npeers, const int32_t *peer_rank, const int64_t *send_count,
                                         const int64_t *recv_count, const double *send, double *recv);
typedef int (*cice_evp_hip_test_reduce_fn)(void *user, int32_t op, void *value);
int cice_evp_hip_set_test_transport(cice_evp_hip_test_xchg_fn xchg, cice_evp_hip_test_reduce_fn reduce, void *user);
/* Host-only (CPU tests): geometry and exchange lists of the marching path for dims->rank.  Every rank's sub-domain
 * must be one rectangle; the rank HOLDS its own cells plus `ext` (even) more on every side that has a neighbour, in strips
 * of `own` <= own_max columns (position of a cell = (storage row * nstrips + strip) * 64 + lane), and after one exchange
 * of the ring of ext + 2 cells ext/2 + 1 passes can follow.  geo14 = {gx0, gy0, nxr, nyr of what it holds, own, nstrips,
 * peers, cells sent, cells received, wraps inside, ext west / east / south / north}; per peer (ascending rank; the rank
 * itself when wrap_inside = 0 on a cyclic dimension it spans) the cells it sends / receives, recv_pos2 = the duplicate
 * position or -1.  Lists may be NULL.                                                                                */
int cice_evp_hip_march_plan(const cice_evp_hip_dims *dims, int32_t own_max, int32_t wrap_inside, int32_t ext, int32_t *geo14,
                            int32_t *peer_rank, int32_t *peer_nsend, int32_t *peer_nrecv, int32_t *send_pos,
                            int32_t *recv_pos1, int32_t *recv_pos2);
/* Host-only (CPU tests): how the marching path shares a tripole / tripoleT grid on one rank between the marched zone and the fold
 * band (cice_amd/csrc/march_plan.h: MarchFold).  ext as above; tyb = tile height of the one-subcycle kernel (2 .. 9).  Rows are
 * global, 0-based, windows half open.  out10 = {zone rows (the zone is rows 0 .. zone-1), band rows H, ext, U-rows per tile row,
 * lowest row the band's tile list covers, ring exchange rectangle -> block layout [lo, hi), block layout -> rectangle [lo, hi),
 * rows the zone's rectangle holds (zone + ext)}; tile_rows (may be NULL) = per local block the tile rows [by0, by1) of the band's
 * list.  Fails (-3) where there is no fold, on several ranks (the one-rank question: the several-rank form is planned by
 * cice_evp_hip_march_layout only), and on a grid too short for a zone under the band.                                     */
int cice_evp_hip_march_fold_plan(const cice_evp_hip_dims *dims, int32_t ext, int32_t tyb, int32_t *out10, int32_t *tile_rows);
/* Host-only (CPU tests): everything the marching path's host decides from the dims and what it may be asked for alone
 * (cice_amd/csrc/march_plan.h: build_march_layout).  ask7 = {own_max, wrap_inside, ext, kpass, seglen, bandseg, tyb}: the test build's
 * switches CICE_EVP_HIP_MARCH_OWN / _SELFX (inverted) / _EXT / _K / _SEG / _BANDSEG and the tile height; ext, kpass = INT32_MIN: not
 * asked for (the rim and pass size rules decide), seglen, bandseg = 0 likewise.  info37 = {ext, ring_valid, kpass, bsx, bsy, nbx, nby, nxr,
 * nyr, ldx, rows, own, nstrips, wrapx, gx0, gy0, ext_w, ext_s, nxo, nyo, nyblk, nblk, seglen, nseg, nitems, peers, cells sent, cells
 * received, band items, rest items, fold band rows, zone rows, entries of org, entries of dup, fold band rows THIS rank holds, ranks
 * that hold some, lowest row the band's tile list covers}.  A tripole / tripoleT grid on several ranks: one zone and one band for the
 * grid (the same fold band rows, zone rows and list row on every rank), the band on the ranks whose blocks reach above the zone; the
 * exchange lists of such a rank also name the corner cells above the zone beside its own columns (march_plan.h).  Tables (any may be NULL; sizes from a
 * first call): blkid [nby][nbx]; org2 [nblocks]{x, y}; dup [nstrips][64] byte offsets; ring5 = send_pos, send_midx [cells sent] then
 * recv_pos1, recv_pos2, recv_midx [cells received]; cuts3 = where each peer's share begins in the send list, then in the receive list,
 * then the peers' ranks (and -1), [peers + 1] each; band4 / rest4 = the work items {strip, y0, y1, 0} of an overlapped exchange pass.  Fails (-3) with the words the
 * library gives for "marching kernel off" where the layout refuses the domain.                                                   */
int cice_evp_hip_march_layout(const cice_evp_hip_dims *dims, const int32_t *ask7, int32_t *info37, int32_t *blkid, int32_t *org2, uint32_t *dup,
                              int32_t *ring5, int32_t *cuts3, int32_t *band4, int32_t *rest4);
/* Host-only (CPU tests): the steps of a call of ndte subcycles (march_plan.h: march_schedule): steps4 = per step {size, ring between ranks
 * travels after it, zone and fold band trade rows after it, last}; a step of size 1 is the leading subcycle of the one-subcycle kernel.
 * *n = number of steps (<= ndte); steps4 may be NULL.                                                                            */
int cice_evp_hip_march_schedule(int32_t ndte, int32_t kpass, int32_t ring_valid, int32_t has_peers, int32_t fold, int32_t *n, int32_t *steps4);
/* Per-CU record of the last on-chip resident launch with 16 x 16 tiles (tools): n <= 2048*8 ints, per CU
 * (index = XCC<<8 | HW_ID[15:8]) {lock, launch stamp, ice-holding waves on SIMD 0..3, 0, 0}.        */
int cice_evp_hip_debug_cuload(int32_t *out, int32_t n);
/* Phase stamps of the last resident launch made under CICE_EVP_HIP_RES_PROF=1 (tools/resident_phases.py):
 * per tile and chunk of 64 cells 8 x uint64 = shader cycles in {ring poll, stress, barrier wait, momentum
 * step + publish, barrier wait}, arrival rank of the workgroup on its CU, hardware wave, active chunks.    */
int cice_evp_hip_debug_prof(uint64_t *out, int32_t ntiles_max);
/* Launch stamps of the same launch (tools/resident_launch_stamps.py): per tile and hardware wave 8 x uint64 = the 100 MHz wall clock at
 * workgroup start, after the per-CU lock, after the lane tables and masks, after the state loads, at the first ring poll's match,
 * at the loop's end, at the write-back's end; chunk the wave took | active chunks of the tile << 8.                                */
int cice_evp_hip_debug_prof_launch(uint64_t *out, int32_t ntiles_max);
/* (word 6 of a chunk's stamps = hardware wave | passes that took the compiler's sqrt / division << 8: a wave of the lean loops makes
 * one stress pass and one or two momentum-step passes per subcycle, each on the range-proved cores or not -- csrc/evp_range_math.h) */
/* The range-proved fp64 square root and division of the lean resident loops (csrc/evp_range_math.h: sqrt_core, div_core) beside the
 * compiler's sqrt and /, element by element on the current device (no cice_evp_hip_init needed): n host values each of x, num, den
 * in; sqrt(x) and num / den by both out; verdict[e] bit 0: x[e] is inside the window the kernels test, bit 1: num[e] and den[e]
 * both are.  Where a bit is set the two forms must agree to the bit.                                                             */
int cice_evp_hip_debug_range_math(int64_t n, const double *x, const double *num, const double *den, double *sqrt_lib, double *sqrt_core,
                                  double *div_lib, double *div_core, uint8_t *verdict);
/* C grid, one-launch kernel: 8 stamps per window of the last launch (CICE_EVP_HIP_CGRID_PROF=1 when the geometry was set):
 * shader-clock cycles at 0 start, 1 / 2 before / after the first workgroup barrier, 3 / 4 the second, 5 level C's arithmetic
 * done, 6 end; 7 = XCC id << 32 | HW_ID.  Returns the number of windows.  tools/cgrid_phases.py */
int cice_evp_hip_debug_cgrid_prof(uint64_t *out, int32_t ntiles_max);
/* The same for the on-chip resident C-grid kernel (cg_res): 32 values per window = 4 waves x 8 phases, shader cycles summed over the
 * last launch: poll | barrier | S | barrier | T | barrier | U + barrier | C.  Returns the number of windows.                       */
int cice_evp_hip_debug_cgres_prof(uint64_t *out, int32_t ntiles_max);
/* How many device allocations the library holds right now, over the B-grid state, the marching path and the C-grid state (what
 * their pools have registered and cice_evp_hip_finalize releases): 0 before cice_evp_hip_init and after cice_evp_hip_finalize. */
int cice_evp_hip_debug_device_allocs(int64_t *count);
/* Host-only: build the plan for `dims` without touching a device (CPU tests). */
int cice_evp_hip_plan_build(const cice_evp_hip_dims *dims);
/* The whole plan built last as int32 values: every member of HaloPlan in declaration order (cice_amd/csrc/halo_plan.h) -- a list as
 * its length, then its entries; the peer lists (peers, cg_peers) as their length, then every peer member by member; cg_fold[0 .. 3];
 * the error text as its length, then its characters.  Returns the number of values; out = NULL: only counts; -1 when n is too small. */
int cice_evp_hip_plan_dump(int32_t *out, int32_t n);
/* Host-only: lane tables of the resident B-grid kernel's rim-wave schedule (csrc/rim_plan.h) for one block of ni x nj cells
   with one ghost cell all round; mask: (ni + 2) x (nj + 2) bytes, bit 0 ice T-cell, bit 1 ice U-cell.  Returns the tile count
   (all out pointers NULL: only that).  Per tile perm[256], uperm[256] (255: none), info8 = {|L_T|, |L_U|, active chunks,
   active chunks of the ice-first packing, ok, tiles per row, tiles per column, 0}, cls[256]. */
int cice_evp_hip_rim_plan(int32_t ni, int32_t nj, int32_t cyclic_ew, int32_t cyclic_ns, const uint8_t *mask, int32_t ntiles_max,
                          uint8_t *perm, uint8_t *uperm, int32_t *info8, uint8_t *cls);
/* Host-only: which instantiation of the resident B-grid kernel a launch runs (csrc/res2_variant.cpp: res2_choose), for n cases that
   share cap (3, 1, 0, -1), logw (4, 5, 6) and hooks (the value of CICE_EVP_HIP_RES_DEBUG: csrc/evp_device.h, EVP_RES2_HOOK_*).
   facts[e] bit 0 strict, 1 neighbours on other GPUs, 2 one block per rank, 3 - 7 the launch carries the seam / T-fold / img3 / rimg /
   rraw table, 8 revp == 0, 9 / 10 the flags WATER_IS_OCN / TBU_ZERO, 11 - 13 COOP is possible for the tables / built / fits the chip,
   14 the rim-wave tables are valid, 15 - 17 the switches RES_COOP / RES_LEAN / RES_RIMU.  chosen[e] bit 0 strict, 1 remote, 2 coop,
   3 lean, 4 rimu, 5 the launch binds rim_plan's tables; logw << 8; (cap + 1) << 16.                                              */
int cice_evp_hip_debug_res2_choose(int64_t n, const uint32_t *facts, int32_t cap, int32_t logw, int32_t hooks, uint32_t *chosen);
/* Host-only: which schedule the C-grid subcycle loop runs (csrc/cgrid_schedule.cpp: cg_choose_schedule), for n rows of 26 facts each
   in the order of CgSchedFacts (csrc/cgrid_schedule.h): one_tab remote tripole tfold geo frame_plan one_items rest_plan rest_items
   by_size rest_scr5 | avg_strength fast | res_mode res_ok | the switches ONE FUSED MARCH_RANKS MARCH_FOLD MARCH_FOLD_RANKS
   MARCH_AVG_STRENGTH MARCH_FOLD_SERIAL STRIP_LAST (the two tri-states: 0, 1 or INT32_MIN = not set) | ndte first synced.
   out: n rows of 7, {kind, nres, fast, geo, serial, strip_last, sync}; kind 0 five phases, 1 three fused launches, 2 cg_one, 3 zone
   marched + frame, 4 ... on the five phases, 5 marched zone + fold band, 6 ... + frame, 7 five phases + cg_res FOLD.            */
int cice_evp_hip_debug_cgrid_choose(int64_t n, const int32_t *facts, int32_t *out);
/* Host-only: 1 where this build holds that instantiation of the kernel (the table of csrc/evp_resident2.hip), else 0. */
int cice_evp_hip_debug_res2_built(int32_t strict, int32_t cap, int32_t logw, int32_t remote, int32_t coop, int32_t lean, int32_t rimu);
int cice_evp_hip_halo_plan(int32_t *counts4, int32_t *local_dst, int32_t *local_src,
                           int32_t *local_sign, int32_t *peer_rank, int32_t *peer_nsend,
                           int32_t *peer_nrecv, int32_t *send_src, int32_t *recv_dst);

/* Tripole (u-fold) part of the plan: counts3 = {seam pairs, pole cells, late copies}.
 * After every velocity update the pair (a,b) of the seam row becomes (xavg, -xavg),
 * pole cells change sign, then the late copies are (re)applied
 * (ice_boundary.F90:1630-1649, 1689-1722).  Lists may be NULL.                  */
int cice_evp_hip_seam_plan(int32_t *counts3, int32_t *seam_a, int32_t *seam_b, int32_t *seam_pole,
                           int32_t *late_dst, int32_t *late_src, int32_t *late_sign);
/* What the mailbox transports use on top of cice_evp_hip_halo_plan's lists, same peer order and
 * lengths as send_src / recv_dst: send_dst = the ghost cell each sent value fills, as an offset
 * into the PEER's array (remote stores need it; no set-up traffic -- every rank enumerates every
 * rank's ghosts); recv_gid = global cell number (ig-1)+nx_global*(jg-1) each received ghost mirrors
 * (probe exchanges).  Lists may be NULL.                                                         */
int cice_evp_hip_peer_plan(int32_t *send_dst, int32_t *recv_gid);
/* What the on-chip kernel uses when the tripole fold row is split over ranks: per peer counts4 = {ghost entries at the head
 * of the send list, of the recv list (raw seam values for the staging slots follow them), seam images out, in}; send_sign =
 * the factor the receiver applies, send-list order; out3 = (seam cell here, ghost cell at the peer, sign) per image the owner
 * feeds with its FINAL value; in3 = (ghost cell here, global column of the seam cell, sign).  Lists may be NULL.        */
int cice_evp_hip_fold_images_plan(int32_t *counts4, int32_t *send_sign, int32_t *out3, int32_t *in3);
/* Factor applied to each received value (+1, or -1 for a ghost cell across the tripole fold), recv-list order. */
int cice_evp_hip_peer_signs(int32_t *recv_sign);
/* Ghost-cell lists of cell-centre fields (T-grid inputs of cice_evp_hip_prep) whose source is on
 * this rank: a[dst] <- (vector kind ? vsign : 1) * a[src], src = -1: 0.  Returns 1 (not an error)
 * when some ghost needs another rank.  Lists may be NULL.                                       */
int cice_evp_hip_center_plan(int32_t *count, int32_t *dst, int32_t *src, int32_t *vsign);
/* Lists behind cice_evp_hip_stress_halo: a1[dst] <- a2[src] for every partner pair (src = -1:
 * fill 0, ice_boundary.F90:7643-7645).  Lists may be NULL.                                     */
int cice_evp_hip_stress_plan(int32_t *count, int32_t *dst, int32_t *src);
/* Lists of the shifted-copy exchange that serves centre-kind fields across a tripole fold whose row is split over ranks
 * (cice_amd/csrc/halo_plan.h): which 0 = cells of row NY-1 where a'(c) = a(c + nx_block + 1) is built, 1 = centre-field
 * ghost cells taken from the exchanged copy, 2 = the stress symmetrisation's; 3, 4 = east-west ghost cells of row NY
 * owned elsewhere and the staging slots (offsets behind the array) a plain exchange leaves their values in.  Returns 1
 * when the fold row is split.                                                                                       */
int cice_evp_hip_fold_split_plan(int32_t which, int32_t *count, int32_t *cells);
/* Flags of the plan, up to n of them: [0] some rank's in-loop velocity exchange crosses the tripole fold or uses
 * seam staging slots -- computed identically on every rank, what collective decisions (cice_evp_hip_halo_mask)
 * hang on; [1] fold_rows (0 none here, 1 all here, 2 shared); [2] stress symmetrisation needs another rank;
 * [3] a cell-centre ghost needs another rank; [4] ... across the fold.  Returns the number written.           */
int cice_evp_hip_plan_flags(int32_t *flags, int32_t n);
/* The per-call shortcut verdicts as the kernels of the next launch see them, up to n words: [0] the B grid's effective flag word
 * (flags & allowed, csrc/evp_device.h: EVP_F_*) after the last upload, prep or set_metrics; [1] the C grid's raw flag word of the
 * last finish_upload (csrc/evp_cgrid.hip: cg_call_setup -- bit 0 water differs from ocean, 1 TbE / TbN nonzero, 2 rheofact other
 * than 1); [2] 1 where the C grid then took its default-configuration kernels (CG.fast); [3] 1 where the last B-grid call ran the
 * on-chip resident kernel in a lean variant.  Returns the number written.                                                        */
int cice_evp_hip_debug_call_flags(uint32_t *out, int32_t n);
/* The C grid on a tripole grid, from the plan of cice_evp_hip_plan_build (cice_amd/csrc/halo_plan.h: cg_*).  For field location
 * loc (0 centre, 1 NE corner, 2 E face, 3 N face) the fold step's entries as cice_evp_hip_cgrid_fold_plan gives them; an
 * operand >= nx_block * ny_block * nblocks is a staging slot (the raw value of another rank's cell).  info4 = {1 if the blocks next
 * to the fold have more than one owner (the same on every rank), staging slots, peers of the C-grid exchange, entries sent}. */
int cice_evp_hip_cgrid_fold_xplan(int32_t loc, int32_t *info4, int32_t *count, int32_t *dst, int32_t *a, int32_t *b, int32_t *flip);
/* ... and that exchange: per peer (ascending rank) peer5 = {rank, entries sent, received, of which ghost cells sent, received};
 * the ghost cells come first in each peer's share, the fold sources (into the peer's staging slots) after them.  send_dst: the
 * cell or staging slot each sent entry fills at the peer; recv_gid: the global cell number (ig-1) + NX*(jg-1) each received
 * entry carries. */
int cice_evp_hip_cgrid_fold_xpeers(int32_t *peer5, int32_t *send_src, int32_t *send_dst, int32_t *recv_dst, int32_t *recv_gid);
/* tripoleT, the stress symmetrisation of the plan of cice_evp_hip_plan_build on ANY rank layout (cice_amd/csrc/fold_prep_plan.h):
 * (dst, src) row NY of _1 / _2 from the partner array, (own_dst, own_src) east-west ghost cells of row NY of _3 / _4 from
 * their own array, (corner_dst, corner_src) the north-west corner ghost cell of a top-row block from the partner's row NY-1.
 * A source >= nx_block * ny_block * nblocks is a staging slot of the C-grid exchange above (the one the centre fold step's
 * entries use for that cell).  info4 = {entries of the three lists, 1 if some rank needs a cell of another rank (the same
 * on every rank: the exchange is then collective)}; lists may be NULL.  Returns 1 where it declines (not tripoleT, an
 * eliminated block among the cells read, a cell the exchange does not carry): cice_evp_hip_last_error says why.          */
int cice_evp_hip_stress_tfold_xplan(int32_t *info4, int32_t *dst, int32_t *src, int32_t *own_dst, int32_t *own_src,
                                    int32_t *corner_dst, int32_t *corner_src);
/* Read-outs of the forcing-layout tests (no entry of their own): cice_evp_hip_prep_fetch serves which = 21, 22 = ss_tltxU,
 * ss_tltyU; cice_evp_hip_cgrid_fetch serves table 2, index 0..3 = strairxE, strairyN, ss_tltxE, ss_tltyN as the last
 * cice_evp_hip_cgrid_prep under a forcing layout other than the default averaged them (every cell).                    */


#ifdef __cplusplus
}
#endif
#endif /* CICE_EVP_HIP_TESTING_H */
