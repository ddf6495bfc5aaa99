// Host-side halo plan: which ghost cell of which local block takes its value
// from where.  Pure C++ (no HIP) so that it can be built and tested on a
// machine without a GPU.
//
// Replaces, for the one field pair the subcycle exchanges (uvel,vvel at NE
// corners, vector kind), what ice_HaloCreate precomputes as address lists
// (infrastructure/comm/mpi/ice_boundary.F90:171-885, type ice_halo :88-126):
//   srcLocalAddr/dstLocalAddr -> local (dst, src, sign) lists
//   sendAddr / recvAddr       -> per-peer send_src / recv_dst lists
// Instead of walking block neighbours direction by direction the plan is
// derived from the *meaning* of a ghost cell: it mirrors the interior cell
// that holds the same global (i,j) (cyclic wrap, tripole fold), or nothing
// (closed/open outer boundary: left untouched, as ice_HaloUpdate does when no
// fillValue is given, :1176-1189).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cice_evp_hip.h"

struct FoldList {              // the C grid's fold step of one field location (build_fold_list below)
    std::vector<int32_t> dst, a, b;
    std::vector<uint8_t> flip;
};

struct HaloBlock {
    int gi0, gj0, gnx, gny;   // interior rectangle in global index space (1-based origin)
    int owner, local;         // owning rank (-1: eliminated land block), local block index
};

struct HaloPeer {
    int rank = -1;
    std::vector<int32_t> send_src;    // offsets into the local (nx,ny,nblocks) array
    std::vector<int32_t> send_dst;    // the ghost cell each entry fills, as an offset into the PEER's array
    std::vector<int32_t> recv_dst;
    std::vector<int8_t> recv_sign;
    std::vector<int32_t> recv_gid;    // global cell number (ig-1) + NX*(jg-1) each ghost mirrors (probe exchange)
    std::vector<int8_t> send_sign;    // factor the receiver applies to entry k (= its recv_sign; +1 for raw seam entries)
    // the first n_ghost_* entries of the send / recv lists are ghost cells; what follows (tripole fold row split over ranks)
    // are RAW seam values travelling into staging slots n_local + t of the receiver
    int n_ghost_send = 0, n_ghost_recv = 0;
    // On-chip kernel with the fold row split over ranks: a ghost image of a seam-row cell takes the FINAL (averaged) value
    // straight from the cell's owner, as one more tagged record after the owner's own averaging -- instead of being finalised
    // from raw pair values as the streaming path does.  fimg_*: cells of this rank (seam row) with the ghost cell at the
    // peer they feed and its sign; fimg_recv_*: this rank's ghost cells fed that way, the global column of the seam cell.
    std::vector<int32_t> fimg_src, fimg_dst;
    std::vector<int8_t> fimg_sign;
    std::vector<int32_t> fimg_recv_dst, fimg_recv_col;
    std::vector<int8_t> fimg_recv_sign;
};

struct HaloPlan {
    int nx_block = 0, ny_block = 0, nblocks = 0;
    std::vector<int32_t> local_dst, local_src;   // src = -1: fill with 0
    std::vector<int8_t> local_sign;
    std::vector<HaloPeer> peers;                  // ascending rank
    // Tripole u-fold seam of NE-corner vector fields (ice_boundary.F90:1630-1649,
    // 1689-1722).  The top physical row lies on the fold: U(i,NY) and U(NX-i,NY) are one
    // point, so after every update the pair is replaced by (xavg, -xavg),
    // xavg = 0.5*(x_i - x_{NX-i}), i = 1..NX/2-1; the two pole points i = NX/2, NX mirror
    // onto themselves and change sign.  Offsets into the local array (both cells of a
    // pair must live on this rank).  `late_*`: ghost copies whose source is a seam-row
    // cell; they are repeated after the seam step so that they carry the averaged value.
    std::vector<int32_t> seam_a, seam_b, seam_pole;
    std::vector<int32_t> late_dst, late_src;
    std::vector<int8_t> late_sign;
    // The same step for ANY rank layout (seam pairs, or a ghost cell and the seam cell it mirrors, on different
    // ranks): one entry per cell this rank must finalise after the velocity exchange -- its own seam-row cells and
    // its ghost images of seam-row cells.  x[dst] = coef * 0.5*(x[a] + (-1)*x[b])   (b >= 0: pair average)
    //                                     x[dst] = coef * x[a]                     (b == -1: pole / unpaired cell)
    // a, b are offsets of RAW values of this subcycle: local cells, or staging slots n_local + t that the exchange
    // fills with the raw value of a seam cell of another rank (`tail` slots; they travel as extra entries of the
    // peers' send / recv lists, after the ghost cells).  All reads precede all writes.
    std::vector<int32_t> fin_dst, fin_a, fin_b;
    std::vector<int8_t> fin_coef;
    int tail = 0;
    // Computed identically on EVERY rank (the enumeration below runs over all ranks): some rank's in-loop velocity
    // exchange carries an entry across the tripole fold (sign -1 from another rank) or a staging slot.  Collective
    // decisions (cice_evp_hip_halo_mask) must hang on this, never on a rank's own lists.
    bool any_fold_exchange = false;
    bool stress_remote = false;                   // the stress symmetrisation needs a top-row cell of another rank
    // tripole: which ranks hold the two physical rows next to the fold (NY-1, NY)?  0: none here, 1: all of them here,
    // 2: shared with other ranks (the C-grid fold step then cannot be done on one rank)
    int fold_rows = 0;
    // ice_HaloUpdate_stress (ice_boundary.F90:7441-7826; evp() after the subcycle loop,
    // ice_dyn_evp.F90:1321-1389): ghost row NY+1 of a cell-centre scalar takes the mirrored top
    // physical row of its PARTNER array, a1(ig, NY+1) <- a2(NX-ig+1, NY); ghost cells whose source
    // block was eliminated are set to 0 (src = -1).  Offsets into the local array.
    std::vector<int32_t> stress_dst, stress_src;
    // tripoleT: the same twelve calls rewrite the top PHYSICAL row instead -- a1(ig, NY) <- a2(NX-ig+2, NY), east-west ghost
    // columns of that row included, the ghost row above untouched (T-fold offsets of ice_boundary.F90:7700-7740; pinned on
    // the reference's own arrays, tests/golden/tript_*.npz).  The calls come in pairs (a1, a2), (a2, a1) and the mirror is an
    // involution, so the second call of a pair puts a2's interior values back where they were: what changes is a1 = the
    // arrays _1 and _2 of each family (stress_dst / stress_src above: cell of row NY <- partner array's mirrored cell), and the
    // east-west ghost cells of row NY of _3 and _4, which end up as plain images of their own array (stress_own_*).
    std::vector<int32_t> stress_own_dst, stress_own_src;
    // ... and one cell of the ghost row above: the north-west corner ghost cell of a top-row block (global column ig) takes
    // a2(NX-ig+2, NY-1) -- in BOTH arrays of a pair, each from the other -- unless ig is NX/2 or NX (0).  Found by the geometry
    // sweep against the reference itself (three blocks across the top row are needed to see it) and pinned there on 60 random
    // layouts; nothing else of that row is touched.
    std::vector<int32_t> stress_corner_dst, stress_corner_src;
    // Ghost cells of CELL-CENTRE fields (the T-grid inputs of evp()'s preparation phase,
    // ice_dyn_evp.F90:413-428, 466-470): same as the velocity lists except across the tripole
    // fold, where a centre cell mirrors column NX-ig+1 of row NY-k+1 (ice_boundary.F90:1689-1722,
    // ioffset -1, joffset 0); center_vsign is the factor for vector kinds (-1 across the fold),
    // scalars always copy.  center_remote: some source lives on another rank (not listed).
    std::vector<int32_t> center_dst, center_src;
    std::vector<int8_t> center_vsign;
    bool tfold = false;                           // ns_boundary_type 'tripoleT'
    // tripoleT, cell-centre fields (the preparation phase): the top PHYSICAL row lies on the fold -- made symmetric pair by
    // pair (i <-> NX-i+2 for i = 2..NX/2; i = 1 and NX/2+1 mirror onto themselves) and rewritten from its mirror, east-west
    // ghost columns included; the ghost row above takes row NY-1 at column NX-i+2 (ice_boundary.F90:1563-1583, 1686-1722).
    // As entries of a two-pass fold step (evp_device.h: EvpCgFoldList): x[dst] = s * 0.5*(x[a] + isign*x[b]) or s * x[a]
    // (b = -1), s = flip ? isign : 1.  center_tf_remote: an operand lives on another rank or in an eliminated block (the
    // device preparation then stays with the host).  The lists above hold the other ghost cells (rows below NY).
    std::vector<int32_t> center_tf_dst, center_tf_a, center_tf_b;
    std::vector<uint8_t> center_tf_flip;
    bool center_tf_remote = false;
    bool center_remote = false;
    bool center_fold_remote = false;              // ... and one of them lies across the tripole fold (centre mirror rule, other rank)
    // Centre-field ghost cells of this rank whose source lies across the fold on ANOTHER rank (fold row split in x), and the
    // same for the stress symmetrisation.  They are filled through the ordinary NE-corner exchange run on a SHIFTED copy:
    // with a'(i, NY-1) = a(i+1, NY) on the owner, the corner rule ghost(ig, NY+1) <- -a'(NX-ig, NY-1) delivers
    // -a(NX-ig+1, NY), the centre rule's source (sign fixed afterwards).  fold_shift_cells: this rank's interior cells of
    // row NY-1 (the shifted copy is built there).
    std::vector<int32_t> center_foldr_dst, stress_foldr_dst, fold_shift_cells;
    // ... and this rank's east-west ghost cells of row NY whose source another rank owns: the velocity exchange does not
    // fill them (images of seam-row cells are finalised from RAW values), but it brings the raw value of the source into
    // a staging slot -- which for a cell-centre field IS the ghost value: a[dst] = a[slot] after the exchange
    std::vector<int32_t> center_seam_dst, center_seam_slot;
    bool fold_split = false;                      // the blocks holding row NY have more than one owner: the same on every rank
                                                  // (the exchanges above are collective)
    // C grid on a tripole grid (u-fold and T-fold).  cg_fold: the fold step of each field location for this rank's blocks, the
    // entries of build_fold_list in its order; an operand is a cell of this rank, a staging slot n_local + t (the RAW value of an
    // interior cell of rows NY-2 .. NY that another rank owns, brought by the exchange of the same exchange point), or -1 / -2
    // (no owner: eliminated block).  Without cg_split it is what build_fold_list gives, cg_tail = 0.
    // cg_split: the blocks next to the fold (rows NY-1, NY; T-fold NY-2 .. NY) have more than one owner -- the same on every rank.
    // Then the C-grid loop exchanges through cg_peers instead of peers: per peer (ascending rank) first the ghost cells of
    // rows up to NY (T-fold NY-1) whose source another rank owns, plain copies (never across the fold: the fold step is the
    // last writer of everything beyond, and reads only interior cells and staging slots), then the fold sources: the union over
    // the four locations of this rank's cells that the peer's fold entries read, into the peer's staging slots (send_dst).
    FoldList cg_fold[4];
    std::vector<HaloPeer> cg_peers;
    int cg_tail = 0;
    bool cg_split = false;
    int cg_fold_ranks = 0;                        // ranks that hold blocks next to the fold
    std::string error;
};

// Returns false and sets plan.error on inconsistent input.
bool build_halo_plan(const cice_evp_hip_dims &d, HaloPlan &plan);

// C grid on a tripole (u-fold) grid: the fold step of one field location (0 centre, 1 NE corner, 2 E face, 3 N face),
// by the meaning of the cells (ice_boundary.F90:1626-1722): one entry for every cell of every local block -- interior
// or ghost -- in the top physical row NY (locations with points ON the fold: NE corner, N face) or in the ghost row
// NY+1 (every location).    x[dst] = s * 0.5*(x[a] + isign*x[b])   b >= 0 (or -2: partner's block eliminated, 0)
//                           x[dst] = s * x[a]                      b == -1 (a == -1: source eliminated, 0)
// s = flip ? isign : 1; isign = -1 for vector kinds.  Sources are interior cells of THIS rank (the blocks holding rows
// NY-1 and NY must all be local).  Host only.  d: a description build_halo_plan accepts (nghost 1, every block's interior at
// ilo = jlo = nghost + 1); this entry checks nothing itself.
void build_fold_list(const cice_evp_hip_dims &d, int loc, FoldList &L);
