// Host-only geometry and exchange plan of the several-subcycles-per-pass path (evp_march.hip) -- pure C++, no HIP, so
// that it can be built and tested on a machine without a GPU (tests/test_multirank_cpu.py).
//
// Every rank's sub-domain must be ONE rectangle of the global index space (CICE's cartesian distributions:
// ice_distribution.F90 create_distrb_cart; any number of blocks per rank as long as they tile a rectangle).  The rank
// holds it in the strip-major layout of evp_host_march.cpp: strips of `own` columns, per (row, strip) a block of 64
// lanes -- with P = MARCH_PLAN_PAD (4): lanes P .. P+own-1 own their columns, lanes 0 .. P-1 and P+own .. 2P+own-1 duplicate
// the neighbouring strips' edge columns (or, for the first / last strip, hold the P halo columns beyond the rectangle).
//
// A pass of the marching kernel that advances the state by k <= P subcycles needs it k cells beyond the rectangle on
// every side.  What replaces the reference's ice_HaloUpdate there (ice_boundary.F90:1066-1760; one-cell ring, every
// subcycle) is one exchange of a P-cell ring every few passes: like build_halo_plan, the lists are derived from the meaning of a halo cell --
// it images the cell with the same global index (cyclic wrap) -- by every rank for every rank, in one canonical
// order, so that sender and receiver agree without any set-up communication.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cice_evp_hip.h"

#ifdef EVP_MARCH_PAD
#define MARCH_PLAN_PAD EVP_MARCH_PAD
#else
#define MARCH_PLAN_PAD 4       // == EVP_MARCH_PAD (evp_device.h; evp_host_march.cpp asserts it)
#endif

struct MarchRect {
    int gx0 = 0, gy0 = 0;      // global index (0-based) of the first owned cell
    int nxr = 0, nyr = 0;      // owned cells
    int own = 0, nstrips = 0;
    bool ok = false;
};

struct MarchPeer {
    int rank = -1;
    // position of a cell in a rank's strip-major buffers: (storage row * nstrips + strip) * 64 + lane; element of field f
    // in a buffer with NF fields per block: ((pos >> 6) * NF + f) * 64 + (pos & 63)
    std::vector<int32_t> send_pos;               // in MY layout: the owner's position of the cell
    std::vector<int32_t> send_col;               // its column x (for the row-major byte mask), row = (pos >> 6) / nstrips
    std::vector<int32_t> recv_pos1, recv_pos2;   // in MY layout: where the value goes; pos2 = its duplicate or -1
    std::vector<int32_t> recv_col, recv_row;     // column x / storage row of the halo cell (byte mask)
};

struct MarchFold;
struct MarchPlan {
    MarchRect me;                                // the rectangle this rank HOLDS: its own cells plus `ext` more on every side that
                                                 // has a neighbour (computed redundantly, so that the ring is exchanged less often)
    MarchRect owned;                             // the cells this rank owns (gx0, gy0, nxr, nyr)
    int ext_w = 0, ext_e = 0, ext_s = 0, ext_n = 0;
    std::vector<MarchRect> all;                  // every rank's OWN rectangle (index = rank; ok = false: rank holds nothing)
    std::vector<char> top;                       // fold band: does the rank's share of the grid reach above the zone (it holds band rows)?
    int band_ranks = 0;                          // ... how many do
    bool wrapx = false;                          // E-W cyclic wrap handled inside the rank (it spans the whole dimension)
    std::vector<int32_t> dup;                    // [nstrips][64]: (strip << 8) | lane of the duplicate of an owner lane's column, -1 none
    std::vector<MarchPeer> peers;                // ascending rank; may contain this rank itself (self-exchange across the seam)
    int n_send = 0, n_recv = 0;
    std::string error;                           // non-empty: this domain cannot use the path (the same verdict on every rank)
};

// own_max: widest strip (<= 64 - 2P = 56); wrap_inside: let a rank that spans a cyclic E-W dimension wrap internally
// (false: the seam is exchanged like any other rank boundary -- with the rank itself; a test hook).
// ext (even, >= 0): every rank also holds -- and advances redundantly -- `ext` cells beyond its own on every side that
// has a neighbour.  One exchange then brings the ring of ext + P cells around the rank's own cells up to date, and
// passes advancing ext + P subcycles in all can follow before the next one: every subcycle costs one cell of validity.
// fold_h > 0 (one rank, tripole / tripoleT): the plan is built for the ZONE of a folded grid -- global rows 0 .. NY - fold_h - 1, a
// rectangle closed in the south with a neighbour in the north.  That neighbour is no rank: it is this process's own fold band
// (MarchFold), so no peer list names it; the rows above the zone's own are filled by the ring exchange of evp_host_march.cpp.
// ranks_fold (build_march_layout only; without it a tripole grid on several ranks is refused): the same zone under ONE band shared by
// the top row of ranks.  Every rank's rectangle is its blocks cut off at row `zone`; a rank whose blocks reach that row has the band --
// its own columns of it -- as its northern neighbour, a rank below has a rank there.  The ext + P columns a top rank holds beyond its
// own continue above the zone (rows zone .. zone + ext + P - 1): those CORNER cells belong to the band of its x-neighbour and travel
// with the rank ring, from the positions of the neighbour's rectangle its own band rows were gathered into.  Refused: band list rows
// (list_row0 .. NY - 1) outside the top row of ranks, a top rank whose share of the zone is thinner than ext + P.
bool build_march_plan(const cice_evp_hip_dims &d, int own_max, bool wrap_inside, int ext, MarchPlan &P, int fold_h = 0,
                      const MarchFold *ranks_fold = nullptr);

// A tripole grid on one rank: two sets of cells with a ring between them.
//   zone  global rows 0 .. zone-1, advanced several subcycles per pass in the strip-major rectangle (which also holds `ext`
//         redundant rows above them and reads a ring of P rows above those);
//   band  global rows zone .. NY-1 and the ghost row beyond the fold, advanced one subcycle at a time in the caller's block
//         layout by the tile kernel over a tile list that also covers ext + P rows below the band's own (list_row0 .. zone-1).
// Every ext + P subcycles the ring is exchanged: rows to_block (zone rows under the band) travel rectangle -> block layout,
// rows to_rect (band rows above the zone) block layout -> rectangle.  In between either side loses one row of validity per
// subcycle, from the bottom of the band's list and from the top of the rectangle.
struct MarchFold {
    int H = 0, zone = 0, ext = 0;
    int trow = 0;                  // U-rows per tile row (tile height - 1)
    int list_row0 = 0;             // the band's tile list covers every row from here up (<= zone - (ext + P))
    int to_block[2] = {0, 0};      // [lo, hi) global rows
    int to_rect[2] = {0, 0};
    std::string error;
};
// tyb: tile height of the one-subcycle kernel (2 .. 9).  H is the smallest ext + P (tripoleT: one more, the zone's ring stays
// below the top physical row), rounded up so that the band's list starts on a tile row of the block that holds it (the same
// tiles run either way; the zone loses the rows).
// several_ranks (build_march_layout only): one zone and one band for the whole grid -- global rows, identical on every rank, from
// the grid's size and ext alone: H = ext + P (+ 1), no snap, because each rank tunes its tile height for itself and tyb is therefore
// not the same everywhere.  Without it several ranks are refused (the one-rank question).
bool build_march_fold(const cice_evp_hip_dims &d, int ext, int tyb, MarchFold &F, bool several_ranks = false);
// tile rows [by0, by1) of a block with `gny` rows whose first row is global row gj0 (0-based) that belong to the band's list
void march_fold_tile_rows(const MarchFold &F, int gj0, int gny, int &by0, int &by1);

// ---- one layout: everything the host of the marching path decides from the dims and a few asked-for integers alone ----
// (evp_host_march.cpp uploads it, allocates by it, and asserts that these agree with evp_device.h)
constexpr int MARCH_PLAN_OWN = 64 - 2 * MARCH_PLAN_PAD, MARCH_PLAN_S_NF = 14, MARCH_PLAN_MAXPEER = 16;
constexpr uint32_t MARCH_PLAN_NODUP = 0xffffffffu;
constexpr int MARCH_ASK_UNSET = INT32_MIN;
struct MarchAsk {                   // what the host may be asked for (the test build's switches)
    int own_max = MARCH_PLAN_OWN;
    bool wrap_inside = true;
    int ext = MARCH_ASK_UNSET;      // redundant rim (rounded down to an even number >= 0); unset: the widest of 12 / 8 / 4 / 0 that fits
    int kpass = MARCH_ASK_UNSET;    // subcycles per pass (2 .. P); unset: by the shortest segment of any rank
    int seglen = 0, bandseg = 0;    // rows per segment / per work item of an early launch; 0: by the rules
    int tyb = 5;                    // tile height of the one-subcycle kernel (the fold band's tiles)
};
struct MarchOrg { int32_t x, y; };                   // as the kernels read them: int2
struct MarchItem { int32_t strip, y0, y1, pad; };    // ... int4 {strip, Y0, Y1, 0}
struct MarchLayout {
    MarchPlan plan;                 // the rectangle the rank holds (plan.me), its own cells (plan.owned), the peers
    MarchFold fold;                 // the fold band of a tripole grid (H == 0: none); on several ranks the same on every rank
    int band_rows = 0, band_ranks = 0;          // rows of the band THIS rank holds (fold.H or 0) | ranks that hold some
    int ext = 0, ring_valid = MARCH_PLAN_PAD;   // the rim; cells beyond the rank's own that are current after an exchange of the
                                                // ring (ext + P): that many subcycles can follow before the next exchange
    int kpass = MARCH_PLAN_PAD;     // subcycles a full pass advances the state by
    int bsx = 0, bsy = 0, nbx = 0, nby = 0;     // the rank's blocks as a grid of bsx x bsy cells (the last column / row may be smaller)
    std::vector<int32_t> blkid;     // [nby][nbx] local block index
    std::vector<MarchOrg> org;      // [nblocks] the block's first interior cell in the rectangle the rank HOLDS
    int ldx = 0, rows = 0;          // row stride of the byte mask, rows of every buffer
    size_t nblk = 0;                // (row, strip) blocks per buffer
    int seglen = 0, nseg = 0, nitems = 0;
    std::vector<uint32_t> dup;      // [nstrips][64] byte offset, from the start of a state row, of the lane's duplicate (or NODUP)
    // the ring: the peers' lists one after the other, the mask's indices of the same cells, where each peer's share begins
    std::vector<int32_t> send_pos, recv_pos1, recv_pos2, send_midx, recv_midx;
    int cut_send[MARCH_PLAN_MAXPEER + 1] = {}, cut_recv[MARCH_PLAN_MAXPEER + 1] = {};
    std::vector<MarchItem> band_items, rest_items;   // (strip, rows) that hold a cell some rank receives | every other one
    std::string why;                // why not (the same verdict, the same words on every rank); L keeps what had been decided by then
};
bool build_march_layout(const cice_evp_hip_dims &d, const MarchAsk &ask, MarchLayout &L);

// ---- one schedule: a call of ndte subcycles as q passes of kpass and one of the remaining 2 .. kpass - 1; a single remaining
// subcycle goes FIRST, through the one-subcycle kernel (size 1).  exch: the ring between ranks travels after the pass -- the next
// one needs more valid cells than are left, or it is the last; fexch: zone and fold band trade rows, never after the last pass.
struct MarchStep { int size; bool exch, fexch, last; };
std::vector<MarchStep> march_schedule(int ndte, int kpass, int ring_valid, bool has_peers, bool fold);
