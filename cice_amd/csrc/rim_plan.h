// Lane tables of the resident B-grid kernel's rim-wave schedule (evp_resident2.hip, RIMU; 16 x 16 tiles): which T-cell and
// which U-cell of a tile every lane of its workgroup holds.  Plain host code, no device calls (rim_plan.cpp).
//
// Positions are trow*16 + tcol.  T-cell (r, c) reads the velocities of U-cells (r-1..r, c-1..c); U-cell (r, c) -- owned by the
// tile for r, c <= 14 inside the block -- reads the stress-divergence partials of T-cells (r..r+1, c..c+1).  Chunk 0 (the 64
// lanes the rim wave takes) holds
//   L_T: every ice T-cell that reads a ring velocity with a producer (cls == 2), and as many further ice T-cells as it takes to
//        keep the tile at the chunk count of the ice-first packing (the depth-1 corner cells first), while L_U stays within 64;
//   L_U: every owned U-cell that reads a partial of a cell of L_T, and every owned U-cell whose record another tile polls or
//        that has a ghost image (they publish every subcycle, ice or not).
// Every other U-cell stays with the lane that holds the T-cell of its position.  Held by exactly one lane is: every ice T-cell, and
// every owned U-cell that does anything in the kernel -- it has ice, or it writes a record (polled or imaged).  An owned U-cell
// with neither may be held by no lane: it sits at the position of a padding lane of chunk 0 (a position without ice that fills the
// chunk up to 64), and the kernel's write-back, records and images are all gated on ice / pub / img.  What follows from the
// closure of L_U:
//   * no U-cell outside L_U reads a T-cell of L_T;
//   * no T-cell of L_T reads the velocity of a U-cell outside L_U (the U-cells T(r, c) reads are the ones that read T(r, c)).
#pragma once
#include <cstdint>
#include <vector>

namespace rim_plan {

constexpr int W = 16, NPOS = 256, NONE = 255;      // NONE: the lane holds no U-cell (position 255 is never one)

struct Tile {
    uint8_t perm[NPOS];        // lane -> T-cell position: a permutation; lanes 0..63 are chunk 0
    uint8_t uperm[NPOS];       // lane -> U-cell position, or NONE
    int n_lt, n_lu;            // |L_T|, |L_U|
    int nact;                  // chunks that hold ice cells or the rim wave's duties: the first nact
    int nact_packed;           // the same under the ice-first packing alone (the schedule without L_U)
    bool ok;                   // false: the tile cannot satisfy the rules; the launch takes the other schedule
};

// cls: 0 T-cell not computed, 1 computed, 2 computed and reads a ring velocity that has a producer; ice: the position's T- or
// U-cell takes part in the loop; uown: the tile owns the position's U-cell; upub: ... and its record is polled or imaged
void tile(const uint8_t *cls, const uint8_t *ice, const uint8_t *uown, const uint8_t *upub, Tile &out);

// One block of ni x nj cells with one ghost cell all round (arrays of (ni + 2) x (nj + 2), row-major; mask bit 0: ice T-cell,
// bit 1: ice U-cell), closed or cyclic in either direction, cut into 16 x 16 tiles that share a row / column of T-cells:
// the geometry classes of every tile, by the rules of resident2_setup for one block on one rank
struct Block {
    int gx, gy;                                    // tiles per row / column
    std::vector<uint8_t> cls, ice, uown, upub;     // [gy * gx][256]
    std::vector<Tile> tiles;
    bool ok;                                       // every tile is
};
// (for the CPU test entry cice_evp_hip_rim_plan only: a second statement of the classes for this simplest layout.  The kernel's
// tables are tile() fed from resident2_setup's own classes and publish map, which the GPU tests cover)
void block(int ni, int nj, bool cyclic_ew, bool cyclic_ns, const uint8_t *mask, Block &out);

}  // namespace rim_plan
