#include "halo_plan.h"

#include <algorithm>
#include <map>
#include <set>

namespace {

// ---- blocks and cells ----
// An interior cell by its global (ig, jg): its owner (-1: none, eliminated land block) and its offset in the owner's array.
struct Cell { int owner = -1; int32_t off = -1; };

struct Table {
    std::vector<HaloBlock> blk;
    // blocks of each rank ordered by local index
    std::map<int, std::vector<int>> by_rank;
    int NX = 0, NY = 0, nx = 0, ng = 0, me = 0;
    size_t plane = 0;
    int ew = 0, ns = 0;
    bool tripole = false, tfold = false;

    explicit Table(const cice_evp_hip_dims &d)
        : NX(d.nx_global), NY(d.ny_global), nx(d.nx_block), ng(d.nghost), me(d.rank), plane((size_t)d.nx_block * d.ny_block),
          ew(d.ew_boundary_type), ns(d.ns_boundary_type), tripole(d.ns_boundary_type == CICE_EVP_BND_TRIPOLE),
          tfold(d.ns_boundary_type == CICE_EVP_BND_TRIPOLET) {}
    void add_local_blocks(const cice_evp_hip_dims &d)           // the table of one rank that describes only itself
    {
        for (int b = 0; b < d.nblocks; ++b)
            blk.push_back({d.iglob0[b], d.jglob0[b], d.ihi[b] - d.ilo[b] + 1, d.jhi[b] - d.jlo[b] + 1, me, b});
    }
    void index_ranks()
    {
        for (size_t k = 0; k < blk.size(); ++k)
            if (blk[k].owner >= 0) by_rank[blk[k].owner].push_back((int)k);
        for (auto &kv : by_rank)
            std::sort(kv.second.begin(), kv.second.end(), [&](int a, int b) { return blk[a].local < blk[b].local; });
    }
    const std::vector<int> &blocks_of(int R) const
    {
        static const std::vector<int> none;
        auto it = by_rank.find(R);
        return it == by_rank.end() ? none : it->second;
    }
    int32_t n_local(int R) const { return (int32_t)(plane * blocks_of(R).size()); }     // cells of R's array: its staging slots follow
    int find(int ig, int jg) const
    {
        for (size_t k = 0; k < blk.size(); ++k) {
            const HaloBlock &b = blk[k];
            if (ig >= b.gi0 && ig < b.gi0 + b.gnx && jg >= b.gj0 && jg < b.gj0 + b.gny) return (int)k;
        }
        return -1;
    }
    // array cell (i, j) of block B, 1-based, ghost ring included (the interior is ng + 1 .. ng + gnx, ng + 1 .. ng + gny)
    int32_t offset(const HaloBlock &B, int i, int j) const { return (int32_t)((size_t)B.local * plane + (size_t)(j - 1) * nx + (i - 1)); }
    Cell cell(int ig, int jg) const
    {
        const int k = find(ig, jg);
        if (k < 0 || blk[k].owner < 0) return Cell();
        const HaloBlock &B = blk[k];
        return Cell{B.owner, offset(B, ng + 1 + (ig - B.gi0), ng + 1 + (jg - B.gj0))};
    }
    bool top_row_block(const HaloBlock &B) const { return B.gj0 + B.gny - 1 == NY; }
    int32_t gid(int ig, int jg) const { return (int32_t)((ig - 1) + (size_t)NX * (jg - 1)); }
    int wrap(int ig) const
    {
        while (ig < 1) ig += NX;
        while (ig > NX) ig -= NX;
        return ig;
    }
    std::set<int> owners_reaching(int j) const                   // the ranks that own a block reaching global row j or beyond
    {
        std::set<int> owners;
        for (const HaloBlock &B : blk)
            if (B.owner >= 0 && B.gj0 + B.gny - 1 >= j) owners.insert(B.owner);
        return owners;
    }
    int first_fold_row() const { return tfold ? NY - 2 : NY - 1; }    // first row the C grid's fold step reads
};

// The one walk over a block's array cells with their global coordinates (ig not wrapped), rows then columns.
enum class Rows {
    Ghost,          // the ghost ring
    GhostAndTop,    // ... and the interior cells of global row NY
    Fold            // global rows NY and NY + 1, interior and ghost cells
};
template <class Body>
void for_cells(const Table &T, const HaloBlock &B, Rows rows, Body &&body)
{
    const int ng = T.ng;
    for (int j = 1; j <= B.gny + 2 * ng; ++j) {
        const int jg = B.gj0 + (j - ng - 1);
        if (rows == Rows::Fold && jg != T.NY && jg != T.NY + 1) continue;
        for (int i = 1; i <= B.gnx + 2 * ng; ++i) {
            const bool interior = i > ng && i <= ng + B.gnx && j > ng && j <= ng + B.gny;
            if (interior && (rows == Rows::Ghost || (rows == Rows::GhostAndTop && jg != T.NY))) continue;
            body(i, j, B.gi0 + (i - ng - 1), jg);
        }
    }
}

// ---- the boundary rule ----
struct Src {
    bool outside = false;   // beyond a closed/open outer boundary: ghost left untouched
    int ig = 0, jg = 0;
    int sign = 1;
};
enum class Field { Corner, Centre };     // NE-corner vector fields (the velocities); cell-centre fields

// Which global cell does the position (ig,jg) of a field mirror?
Src resolve(const Table &T, Field field, int ig, int jg)
{
    Src s;
    const int NX = T.NX, NY = T.NY;
    const bool corner = field == Field::Corner;
    if (ig < 1 || ig > NX) {
        if (T.ew == CICE_EVP_BND_CYCLIC) ig = (ig < 1) ? ig + NX : ig - NX;
        else s.outside = true;
    }
    if (jg < 1) {
        if (T.ns == CICE_EVP_BND_CYCLIC) jg += NY;
        else s.outside = true;
    } else if (jg > NY) {
        if (T.ns == CICE_EVP_BND_CYCLIC) jg -= NY;
        else if (T.tfold && corner && !s.outside) {
            // T-fold, NE-corner vector field (ice_boundary.F90:1563-1622 offsets (0, 1), copy-out :1686-1722 with the
            // buffer addresses of :8135-8159): ghost(ig, NY+1) <- - a(NX-ig+1, NY-2)
            ig = NX - ig + 1;
            jg = NY - 2;
            s.sign = -1;
        } else if (T.tripole && !s.outside) {
            // u-fold mirror of an NE-corner vector field (ice_blocks.F90:423-424;
            // copy-out offsets (1,1) and isign = -1, ice_boundary.F90:1555-1556,1632-1633):
            //   ghost(ig, NY+k) <- - a(NX-ig, NY-k)
            // of a cell-centre field (ice_boundary.F90:1689-1722, ioffset -1, joffset 0):
            //   ghost(ig, NY+k) <- - a(NX-ig+1, NY-k+1)
            const int k = jg - NY, shift = corner ? 0 : 1;
            ig = NX - ig + shift;
            if (ig < 1) ig += NX;
            jg = NY - k + shift;
            s.sign = -1;
        } else s.outside = true;      // (tripoleT: no centre lists -- the preparation stays with the host)
    }
    else if (jg == NY && T.tfold && corner && !s.outside) {
        // ... and the top physical row itself (interior cells and their east-west ghost columns) is the image of row
        // NY-1: a(ig, NY) <- - a(NX-ig+1, NY-1); nothing is averaged at this location
        ig = NX - ig + 1;
        jg = NY - 1;
        s.sign = -1;
    }
    s.ig = ig;
    s.jg = jg;
    return s;
}

// ---- what travels between ranks ----
// "Rank R needs the cell c of another rank at its position dst": the receiver appends to its recv lists, the cell's owner to its
// send lists.  Every rank runs the same enumeration for every rank R, so a value R needs appears at the same position of R's recv
// list and of its owner's send list -- the order of these calls is the whole contract between ranks, no set-up traffic.
struct Peers {
    int me;
    std::map<int, HaloPeer> of;
    explicit Peers(int me_) : me(me_) {}
    HaloPeer &peer(int r)
    {
        HaloPeer &p = of[r];
        p.rank = r;
        return p;
    }
    void need(int R, const Cell &c, int32_t dst, int sign, int32_t gid)
    {
        if (R == me) {
            HaloPeer &p = peer(c.owner);
            p.recv_dst.push_back(dst);
            p.recv_sign.push_back((int8_t)sign);
            p.recv_gid.push_back(gid);
        } else if (c.owner == me) {
            HaloPeer &p = peer(R);
            p.send_src.push_back(c.off);
            p.send_dst.push_back(dst);
            p.send_sign.push_back((int8_t)sign);
        }
    }
    void ghost_entries_end_here()        // what the lists hold so far are ghost cells; staging slots follow
    {
        for (auto &kv : of) { kv.second.n_ghost_send = (int)kv.second.send_src.size(); kv.second.n_ghost_recv = (int)kv.second.recv_dst.size(); }
    }
    std::vector<HaloPeer> list() const   // ascending rank
    {
        std::vector<HaloPeer> v;
        for (const auto &kv : of) v.push_back(kv.second);
        return v;
    }
};

// Staging slots n_local + t of rank R: the raw value of an interior cell another rank owns; the first use of a cell allocates
// its slot and records the transfer.
struct Staging {
    const Table &T;
    Peers &peers;
    int R;
    int32_t base;
    std::map<int32_t, int32_t> slot_of;                  // global cell -> staging slot of R
    Staging(const Table &T_, Peers &peers_, int R_) : T(T_), peers(peers_), R(R_), base(T_.n_local(R_)) {}
    int count() const { return (int)slot_of.size(); }
    // the operand that stands, at R, for the raw value of interior cell (ig, jg): its offset, a staging slot, or -1 (no owner)
    int32_t operand(int ig, int jg)
    {
        const Cell c = T.cell(ig, jg);
        if (c.owner < 0) return -1;
        if (c.owner == R) return c.off;
        const int32_t gid = T.gid(ig, jg);
        auto it = slot_of.find(gid);
        if (it != slot_of.end()) return it->second;
        const int32_t slot = base + (int32_t)slot_of.size();
        slot_of[gid] = slot;
        peers.need(R, c, slot, 1, gid);
        return slot;
    }
};

// The fold step of the C grid for the blocks of rank R: one entry per cell of rows NY / NY+1, ghost columns included, in block, row,
// column order.  own(ig, jg), ig in 1..NX, jg in NY-2 .. NY: the operand that stands for the raw value of interior cell (ig, jg) -- an
// offset, a staging slot, or -1 (no owner).
// u-fold (ice_boundary.F90:1626-1722): row NY of NE-corner fields pairs i <-> NX-i (poles NX/2, NX), of N-face fields i <-> NX+1-i;
// the ghost row NY+1 mirrors with offsets (0,0) centre, (1,1) NE corner, (1,0) E face, (0,1) N face.  A point ON the fold is
// averaged with its partner even when the partner's block was eliminated (the buffer holds 0: b = -2).
// T-fold (ice_boundary.F90:1563-1622 offsets and symmetrisation, :1686-1722 copy-out): rows NY and NY+1 take column
// NX-ig+1-ioffset of the rows NY-joffset and NY-1-joffset, offsets (ioffset, joffset) = centre (-1, 0), NE corner (0, 1), E face
// (0, 0), N face (-1, 1); centre and E-face fields lie ON the fold: their top row is made symmetric first (pairs i <-> NX-i+2,
// i = 2..NX/2, resp. i <-> NX+1-i, i = 1..NX/2) -- an entry then holds the pair in the reference's order (a = the lower column)
// and flip says which half the destination is.
template <class Own>
void fold_entries(const Table &T, int R, int loc, Own &&own, FoldList &L)
{
    const int NX = T.NX, NY = T.NY;
    auto add = [&](int dd, int aa, int bb, int fl) { L.dst.push_back(dd); L.a.push_back(aa); L.b.push_back(bb); L.flip.push_back((uint8_t)fl); };
    auto pair = [&](int dd, int ia, int ib, int fl) {
        const int pa = own(T.wrap(ia), NY), pb = own(T.wrap(ib), NY);
        add(dd, pa, pb >= 0 ? pb : -2, fl);
    };
    const int ioff = (loc == 0 || loc == 3) ? -1 : 0, joff = (loc == 1 || loc == 3) ? 1 : 0;   // (T-fold)
    const bool on_fold = (loc == 0 || loc == 2);
    for (int kb : T.blocks_of(R))
        for_cells(T, T.blk[kb], Rows::Fold, [&](int i, int j, int ig_raw, int jg) {
            const int ig = T.wrap(ig_raw);
            const int dd = T.offset(T.blk[kb], i, j);
            if (T.tfold) {
                const int m = T.wrap(NX - ig + 1 - ioff);
                if (on_fold && jg == NY && m != ig) {      // a pair of the symmetrised row
                    const int lo = std::min(ig, m), hi = std::max(ig, m);
                    pair(dd, lo, hi, ig == lo ? 0 : 1);
                } else {
                    add(dd, own(m, (jg == NY ? NY : NY - 1) - joff), -1, 1);
                }
                return;
            }
            if (jg == NY) {
                if (loc == 1) {                           // NE corner: pairs i <-> NX-i, poles NX/2 and NX
                    if (ig == NX / 2 || ig == NX) add(dd, own(ig, NY), -1, 1);
                    else if (ig < NX / 2) pair(dd, ig, NX - ig, 0);
                    else pair(dd, NX - ig, ig, 1);
                } else if (loc == 3) {                    // N face: pairs i <-> NX+1-i
                    if (ig <= NX / 2) pair(dd, ig, NX + 1 - ig, 0);
                    else pair(dd, NX + 1 - ig, ig, 1);
                }
                return;                                   // centre / E face: the top row is an ordinary row
            }
            const int is = (loc == 0 || loc == 3) ? NX - ig + 1 : NX - ig;
            add(dd, own(T.wrap(is), (loc == 0 || loc == 2) ? NY : NY - 1), -1, 1);
        });
}

// ---- the steps of build_halo_plan, in its order ----

// 1. checks of the description itself; tfold
bool check_dims(const cice_evp_hip_dims &d, HaloPlan &plan)
{
    if (d.nghost != 1) {
        plan.error = "nghost must be 1 (ice_blocks.F90:47)";
        return false;
    }
    plan.tfold = d.ns_boundary_type == CICE_EVP_BND_TRIPOLET;
    if ((plan.tfold || d.ns_boundary_type == CICE_EVP_BND_TRIPOLE) && (d.nx_global % 2 != 0 || d.ew_boundary_type != CICE_EVP_BND_CYCLIC)) {
        plan.error = "tripole needs an even nx_global and a cyclic east-west boundary";
        return false;
    }
    // (tripoleT on several ranks: the images of the top row are INTERIOR cells -- receive lists may name them; the exchange
    // then has to follow the launch that computes them, never ride in it: evp_host_loop.cpp use_riding_exchange / use_overlap)
    return true;
}

// 2. the table of all blocks, and the local description checked against it
bool make_table(const cice_evp_hip_dims &d, Table &T, std::string &error)
{
    if (d.gi0 != nullptr && d.nblocks_tot > 0) {
        for (int k = 0; k < d.nblocks_tot; ++k)
            T.blk.push_back({d.gi0[k], d.gj0[k], d.gnx[k], d.gny[k], d.gowner[k], d.glocal[k]});
    } else {
        if (d.nranks != 1) {
            error = "global block table required when nranks > 1";
            return false;
        }
        T.add_local_blocks(d);
    }
    T.index_ranks();
    const std::vector<int> &mine = T.blocks_of(T.me);
    if ((int)mine.size() != d.nblocks) {
        error = "global block table disagrees with nblocks of this rank";
        return false;
    }
    const int ng = T.ng;
    for (int b = 0; b < d.nblocks; ++b) {
        const HaloBlock &B = T.blk[mine[b]];
        if (d.ilo[b] != ng + 1 || d.jlo[b] != ng + 1 || B.local != b || B.gi0 != d.iglob0[b] ||
            B.gj0 != d.jglob0[b] || B.gnx != d.ihi[b] - d.ilo[b] + 1 ||
            B.gny != d.jhi[b] - d.jlo[b] + 1 || d.ihi[b] + ng > d.nx_block || d.jhi[b] + ng > d.ny_block) {
            error = "local block geometry inconsistent with the global block table";
            return false;
        }
    }
    return true;
}

// fold_rows: who owns the blocks that hold the rows next to the fold (tripoleT NY-2 .. NY: the C grid's fold step reads all three;
// tripole NY-1 / NY); fold_split (tripole): the blocks whose top row IS NY have more than one owner
void fill_fold_rows_and_fold_split(const Table &T, HaloPlan &plan)
{
    if (!T.tripole && !T.tfold) return;
    const std::set<int> owners = T.owners_reaching(T.first_fold_row());
    const bool mine = owners.count(T.me) != 0, others = owners.size() > (mine ? 1u : 0u);
    plan.fold_rows = !mine ? 0 : (others ? 2 : 1);
    if (!T.tripole) return;
    int first = -1;
    for (const HaloBlock &B : T.blk) {
        if (B.owner < 0 || !T.top_row_block(B)) continue;
        if (first < 0) first = B.owner;
        else if (B.owner != first) plan.fold_split = true;
    }
}

struct GhostSeam { int R; int32_t dst; int sig; int sign; };   // a ghost cell (of rank R) that mirrors seam-row cell sig, times sign

// 3. velocity ghost cells: local_*, late_*, the ghost entries of the peers' send / recv lists, fimg_*, any_fold_exchange
// Enumerate the ghost cells of every rank in one canonical order (local
// block index, then j, then i).  The receiver keeps entries whose source it
// does not own in recv lists; the owner of the source, running the very same
// enumeration, appends the matching cell to its send list -- so both lists
// have identical order without any set-up communication.
void fill_velocity_ghost_cells(const Table &T, HaloPlan &plan, Peers &peers, std::vector<GhostSeam> &ghost_seam)
{
    const int me = T.me;
    auto local = [&](int32_t dst, int32_t src, int sign) {
        plan.local_dst.push_back(dst);
        plan.local_src.push_back(src);
        plan.local_sign.push_back((int8_t)sign);
    };
    for (const auto &kv : T.by_rank) {
        const int R = kv.first;
        for (int kb : kv.second) {
            const HaloBlock &B = T.blk[kb];
            // (tripoleT: the top physical row is a destination of the halo update as well)
            for_cells(T, B, T.tfold ? Rows::GhostAndTop : Rows::Ghost, [&](int i, int j, int ig, int jg) {
                const Src s = resolve(T, Field::Corner, ig, jg);
                if (s.outside) return;
                const int32_t dst = T.offset(B, i, j);
                const Cell c = T.cell(s.ig, s.jg);
                if (c.owner < 0) {
                    // eliminated land block: reference fills with 0 (srcBlock == 0)
                    if (R == me) local(dst, -1, 1);
                    return;
                }
                const bool src_on_seam = T.tripole && s.jg == T.NY;
                if (src_on_seam) {
                    // finalised after the exchange from RAW pair values (fin lists below); the plain copy only
                    // stays in the local lists (late_*: single-rank form of the same step)
                    ghost_seam.push_back({R, dst, s.ig, s.sign});
                    if (c.owner != R) {
                        // (on-chip kernel: the owner's final value as a record of its own, see halo_plan.h)
                        if (c.owner == me) {
                            HaloPeer &p = peers.peer(R);
                            p.fimg_src.push_back(c.off); p.fimg_dst.push_back(dst); p.fimg_sign.push_back((int8_t)s.sign);
                        } else if (R == me) {
                            HaloPeer &p = peers.peer(c.owner);
                            p.fimg_recv_dst.push_back(dst); p.fimg_recv_col.push_back(s.ig); p.fimg_recv_sign.push_back((int8_t)s.sign);
                        }
                        return;
                    }
                }
                if (c.owner != R) {
                    if (s.sign < 0) plan.any_fold_exchange = true;      // (while walking EVERY rank: the same on every rank)
                    peers.need(R, c, dst, s.sign, T.gid(s.ig, s.jg));
                } else if (R == me) {
                    local(dst, c.off, s.sign);
                    if (src_on_seam) {
                        plan.late_dst.push_back(dst);
                        plan.late_src.push_back(c.off);
                        plan.late_sign.push_back((int8_t)s.sign);
                    }
                }
            });
        }
    }
}

// 4. cell-centre fields, ghosts of this rank's blocks: center_dst / src / vsign, center_remote, center_fold_remote, center_foldr_dst
void fill_center(const Table &T, HaloPlan &plan)
{
    for (int kb : T.blocks_of(T.me)) {
        const HaloBlock &B = T.blk[kb];
        for_cells(T, B, Rows::Ghost, [&](int i, int j, int ig, int jg) {
            const Src s = resolve(T, Field::Centre, ig, jg);
            if (s.outside) return;
            const int32_t dst = T.offset(B, i, j);
            const Cell c = T.cell(s.ig, s.jg);
            if (c.owner >= 0 && c.owner != T.me) {
                plan.center_remote = true;
                if (s.sign < 0) {
                    plan.center_fold_remote = true;
                    plan.center_foldr_dst.push_back(dst);
                }
                return;
            }
            plan.center_dst.push_back(dst);
            plan.center_src.push_back(c.off);                              // (eliminated land block: -1, 0)
            plan.center_vsign.push_back((int8_t)(c.owner < 0 ? 1 : s.sign));
        });
    }
}

// 5. tripoleT, cell-centre fields: rows NY (on the fold) and NY+1 of this rank's blocks, ghost columns included: center_tf_*
void fill_center_tfold(const Table &T, HaloPlan &plan)
{
    const int NX = T.NX, NY = T.NY;
    auto mine = [&](int ig, int jg) -> int32_t {
        const Cell c = T.cell(ig, jg);
        if (c.owner != T.me) plan.center_tf_remote = true;
        return c.owner == T.me ? c.off : -1;
    };
    for (int kb : T.blocks_of(T.me)) {
        const HaloBlock &B = T.blk[kb];
        for_cells(T, B, Rows::Fold, [&](int i, int j, int ig_raw, int jg) {
            const int ig = T.wrap(ig_raw), m = T.wrap(NX - ig + 2);
            int32_t a, b = -1;
            uint8_t flip = 1;
            if (jg == NY + 1) a = mine(m, NY - 1);
            else if (ig == 1 || ig == NX / 2 + 1) a = mine(ig, NY);
            else if (ig <= NX / 2) { a = mine(ig, NY); b = mine(m, NY); flip = 0; }
            else { a = mine(m, NY); b = mine(ig, NY); }
            plan.center_tf_dst.push_back(T.offset(B, i, j));
            plan.center_tf_a.push_back(a);
            plan.center_tf_b.push_back(b);
            plan.center_tf_flip.push_back(flip);
        });
    }
}

// 6a. tripole: seam pairs with both halves on this rank (single-rank form; on-chip kernel): seam_a / seam_b, seam_pole
void fill_seam_pairs(const Table &T, HaloPlan &plan)
{
    const int NX = T.NX, NY = T.NY;
    for (int ig = 1; ig <= NX; ++ig) {
        const Cell a = T.cell(ig, NY);
        if (ig == NX / 2 || ig == NX) {
            if (a.owner == T.me) plan.seam_pole.push_back(a.off);
            continue;
        }
        if (ig > NX / 2 - 1) continue;      // pairs are enumerated from their low index
        const Cell b = T.cell(NX - ig, NY);
        if (a.owner != T.me || b.owner != T.me) continue;
        plan.seam_a.push_back(a.off);
        plan.seam_b.push_back(b.off);
    }
}

// 6b. tripole, general form: fin_*, tail, center_seam_*, the staging entries of the peers' lists (and any_fold_exchange with them).
// What every rank R must finalise, and which raw seam values of other ranks it needs for that.  Every rank runs the same
// enumeration for every R, so that a needed value appears at the same position of R's recv list and of its owner's send list.
void fill_seam_finalisation(const Table &T, HaloPlan &plan, Peers &peers, const std::vector<GhostSeam> &ghost_seam)
{
    const int NX = T.NX, NY = T.NY, me = T.me;
    for (const auto &kv : T.by_rank) {
        const int R = kv.first;
        Staging staging(T, peers, R);
        auto ref = [&](int ig) { return staging.operand(ig, NY); };   // at R, the RAW value of seam cell (ig, NY); -1: eliminated
        auto finalise = [&](int32_t dst, int sig, int sign) {   // dst takes sign * (final value of seam cell sig)
            int32_t fa, fb = -1;
            int coef = sign;
            if (sig == NX / 2 || sig == NX) {
                fa = ref(sig);
                coef = -sign;                                   // pole: x <- -x
            } else {
                const int lo = std::min(sig, NX - sig), hi = NX - lo;
                const int32_t ra = ref(lo), rb = ref(hi);
                if (ra < 0 || rb < 0) { fa = ref(sig); }        // partner eliminated: nothing to average
                else { fa = ra; fb = rb; if (sig == hi) coef = -sign; }
            }
            if (R == me && fa >= 0) {
                plan.fin_dst.push_back(dst);
                plan.fin_a.push_back(fa);
                plan.fin_b.push_back(fb);
                plan.fin_coef.push_back((int8_t)coef);
            }
        };
        for (int ig = 1; ig <= NX; ++ig) {       // R's own seam-row cells
            const Cell c = T.cell(ig, NY);
            if (c.owner == R) finalise(c.off, ig, 1);
        }
        for (const GhostSeam &g : ghost_seam)    // R's ghost images of seam-row cells
            if (g.R == R) {
                finalise(g.dst, g.sig, g.sign);
                if (R == me && g.sign > 0) {     // an east-west image in row NY itself: for centre fields, the raw value
                    const int32_t slot = ref(g.sig);
                    if (slot >= staging.base) { plan.center_seam_dst.push_back(g.dst); plan.center_seam_slot.push_back(slot); }
                }
            }
        if (staging.count() > 0) plan.any_fold_exchange = true;
        if (R == me) plan.tail = staging.count();
    }
}

// 7a. tripole, stress symmetrisation (cell-centre fold: partner column NX-ig+1): the ghost row NY+1 of this rank's top-row blocks:
// stress_dst / stress_src, stress_foldr_dst, stress_remote
void fill_stress_ufold(const Table &T, HaloPlan &plan)
{
    for (int kb : T.blocks_of(T.me)) {
        const HaloBlock &B = T.blk[kb];
        if (!T.top_row_block(B)) continue;
        for_cells(T, B, Rows::Fold, [&](int i, int j, int ig, int jg) {
            if (jg != T.NY + 1) return;
            const Cell c = T.cell(T.NX - T.wrap(ig) + 1, T.NY);
            if (c.owner >= 0 && c.owner != T.me) {
                // partner on another rank: through the exchange of a shifted copy (halo_plan.h)
                plan.stress_remote = true;
                plan.stress_foldr_dst.push_back(T.offset(B, i, j));
                return;
            }
            plan.stress_dst.push_back(T.offset(B, i, j));
            plan.stress_src.push_back(c.off);
        });
    }
}

// 7b. tripoleT, stress symmetrisation (halo_plan.h): row NY of this rank's top-row blocks and the north-west corner ghost cell:
// stress_dst / stress_src, stress_own_*, stress_corner_*, stress_remote
void fill_stress_tfold(const Table &T, HaloPlan &plan)
{
    const int NX = T.NX, NY = T.NY, ng = T.ng;
    // (a partner on another rank, or in an eliminated land block -- where the shortcut of the call pairs does not hold:
    // the symmetrisation then stays with the host)
    auto mine = [&](int ig, int jg) -> int32_t {
        const Cell c = T.cell(ig, jg);
        if (c.owner != T.me) plan.stress_remote = true;
        return c.owner == T.me ? c.off : -1;
    };
    for (int kb : T.blocks_of(T.me)) {
        const HaloBlock &B = T.blk[kb];
        if (!T.top_row_block(B)) continue;
        const int ig_nw = T.wrap(B.gi0 - 1);                // the north-west corner ghost cell
        if (ig_nw != NX / 2 && ig_nw != NX) {
            const int32_t src = mine(T.wrap(NX - ig_nw + 2), NY - 1);
            plan.stress_corner_dst.push_back(T.offset(B, ng, ng + B.gny + 1));
            plan.stress_corner_src.push_back(src);
        }
        for_cells(T, B, Rows::Fold, [&](int i, int j, int ig_raw, int jg) {
            if (jg != NY) return;
            const int ig = T.wrap(ig_raw);
            const int32_t dst = T.offset(B, i, j), src = mine(T.wrap(NX - ig + 2), NY);
            plan.stress_dst.push_back(dst);
            plan.stress_src.push_back(src);
            if (i <= ng || i > ng + B.gnx) {              // an east-west ghost cell: image of its own array's cell
                const int32_t own = mine(ig, NY);
                plan.stress_own_dst.push_back(dst);
                plan.stress_own_src.push_back(own);
            }
        });
    }
}

// 8. tripole, where the shifted copies are built: this rank's interior cells of row NY-1 whose block also holds row NY: fold_shift_cells
void fill_fold_shift_cells(const Table &T, HaloPlan &plan)
{
    for (int kb : T.blocks_of(T.me)) {
        const HaloBlock &B = T.blk[kb];
        if (!T.top_row_block(B) || B.gny < 2) continue;
        for (int i = T.ng + 1; i <= T.ng + B.gnx; ++i) plan.fold_shift_cells.push_back(T.offset(B, i, T.ng + B.gny - 1));
    }
}

// 9. tripole, ghost cells whose source block was eliminated: ice_HaloUpdate_stress writes the fill value
// (srcBlock == 0, ice_boundary.F90:7643-7645) -- the same cells the velocity plan zero-fills: more of stress_dst / stress_src
void fill_stress_zero_fill(HaloPlan &plan)
{
    std::set<int32_t> listed(plan.stress_dst.begin(), plan.stress_dst.end());
    for (size_t k = 0; k < plan.local_dst.size(); ++k)
        if (plan.local_src[k] < 0 && listed.insert(plan.local_dst[k]).second) {
            plan.stress_dst.push_back(plan.local_dst[k]);
            plan.stress_src.push_back(-1);
        }
}

// 10. The C grid's fold step and, when the blocks next to the fold have more than one owner, its exchange lists (halo_plan.h:
// cg_*).  Every rank runs the same enumeration for every rank R, as above.
void fill_cg_fold(const Table &T, HaloPlan &plan)
{
    const int me = T.me;
    plan.cg_fold_ranks = (int)T.owners_reaching(T.first_fold_row()).size();
    plan.cg_split = plan.cg_fold_ranks > 1;
    Peers peers(me);
    if (plan.cg_split) {
        // ghost cells of rows up to NY (T-fold NY-1) whose source another rank owns: plain copies.  The fold step writes
        // everything above (and, u-fold, the east-west ghost cells of row NY of NE-corner / N-face fields, after this copy)
        const int jmax = T.tfold ? T.NY - 1 : T.NY;
        for (const auto &kv : T.by_rank)
            for (int kb : kv.second) {
                const HaloBlock &B = T.blk[kb];
                for_cells(T, B, Rows::Ghost, [&](int i, int j, int ig, int jg) {
                    if (jg > jmax) return;
                    const Src s = resolve(T, Field::Corner, ig, jg);
                    if (s.outside) return;
                    const Cell c = T.cell(s.ig, s.jg);
                    if (c.owner < 0 || c.owner == kv.first) return;   // (zero fill / local image)
                    peers.need(kv.first, c, T.offset(B, i, j), 1, T.gid(s.ig, s.jg));
                });
            }
        peers.ghost_entries_end_here();
    }
    for (const auto &kv : T.by_rank) {
        const int R = kv.first;
        if (R != me && !plan.cg_split) continue;
        Staging staging(T, peers, R);
        for (int loc = 0; loc < 4; ++loc) {
            FoldList L;
            fold_entries(T, R, loc, [&](int ig, int jg) { return staging.operand(ig, jg); }, L);
            if (R == me) plan.cg_fold[loc] = L;
        }
        if (R == me) plan.cg_tail = staging.count();
    }
    plan.cg_peers = peers.list();
}

}  // namespace

bool build_halo_plan(const cice_evp_hip_dims &d, HaloPlan &plan)
{
    plan = HaloPlan();
    plan.nx_block = d.nx_block;
    plan.ny_block = d.ny_block;
    plan.nblocks = d.nblocks;
    if (!check_dims(d, plan)) return false;
    Table T(d);
    if (!make_table(d, T, plan.error)) return false;
    fill_fold_rows_and_fold_split(T, plan);

    Peers peers(T.me);
    std::vector<GhostSeam> ghost_seam;           // ghost cells (of any rank) that mirror a seam-row cell, canonical order
    fill_velocity_ghost_cells(T, plan, peers, ghost_seam);
    peers.ghost_entries_end_here();
    plan.peers = peers.list();                   // (the tripole section may append staging entries and rebuilds this)
    fill_center(T, plan);
    if (T.tfold) fill_center_tfold(T, plan);
    if (T.tripole) {
        fill_seam_pairs(T, plan);
        fill_seam_finalisation(T, plan, peers, ghost_seam);
        plan.peers = peers.list();
        fill_stress_ufold(T, plan);
    }
    if (T.tfold) fill_stress_tfold(T, plan);
    if (T.tripole) {
        fill_fold_shift_cells(T, plan);
        fill_stress_zero_fill(plan);
    }
    if (T.tripole || T.tfold) fill_cg_fold(T, plan);
    return true;
}

void build_fold_list(const cice_evp_hip_dims &d, int loc, FoldList &L)
{
    L = FoldList();
    Table T(d);                                  // this rank's blocks only: every source is an interior cell of this rank
    T.add_local_blocks(d);
    T.index_ranks();
    fold_entries(T, T.me, loc, [&](int ig, int jg) { return T.cell(ig, jg).off; }, L);
}
