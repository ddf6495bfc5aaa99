#include "fold_prep_plan.h"

#include <algorithm>
#include <map>

namespace {

struct Blocks {
    std::vector<HaloBlock> blk;
    int NX, NY, nx, ng, me;
    size_t plane;

    explicit Blocks(const cice_evp_hip_dims &d)
        : NX(d.nx_global), NY(d.ny_global), nx(d.nx_block), ng(d.nghost), me(d.rank), plane((size_t)d.nx_block * d.ny_block)
    {
        if (d.gi0 != nullptr && d.nblocks_tot > 0) {
            for (int k = 0; k < d.nblocks_tot; ++k) blk.push_back({d.gi0[k], d.gj0[k], d.gnx[k], d.gny[k], d.gowner[k], d.glocal[k]});
        } else {
            for (int b = 0; b < d.nblocks; ++b)
                blk.push_back({d.iglob0[b], d.jglob0[b], d.ihi[b] - d.ilo[b] + 1, d.jhi[b] - d.jlo[b] + 1, me, b});
        }
        // each rank's blocks by local index, ranks ascending: the order of build_halo_plan's lists
        std::stable_sort(blk.begin(), blk.end(), [](const HaloBlock &a, const HaloBlock &b) {
            return a.owner != b.owner ? a.owner < b.owner : a.local < b.local;
        });
    }
    int wrap(int ig) const
    {
        while (ig < 1) ig += NX;
        while (ig > NX) ig -= NX;
        return ig;
    }
    int32_t offset(const HaloBlock &B, int i, int j) const { return (int32_t)((size_t)B.local * plane + (size_t)(j - 1) * nx + (i - 1)); }
    const HaloBlock *find(int ig, int jg) const
    {
        for (const HaloBlock &b : blk)
            if (ig >= b.gi0 && ig < b.gi0 + b.gnx && jg >= b.gj0 && jg < b.gj0 + b.gny) return &b;
        return nullptr;
    }
};

}  // namespace

void build_stress_tfold_xplan(const cice_evp_hip_dims &d, const HaloPlan &P, StressTfoldXPlan &X)
{
    X = StressTfoldXPlan();
    if (!P.tfold) {
        X.why = "not a tripoleT grid";
        return;
    }
    const Blocks T(d);
    const int NX = T.NX, NY = T.NY, ng = T.ng;
    // the staging slots of this rank: the fold sources ride behind the ghost cells of each peer's list
    std::map<int32_t, int32_t> slot_of;
    for (const HaloPeer &p : P.cg_peers)
        for (size_t k = (size_t)p.n_ghost_recv; k < p.recv_dst.size(); ++k) slot_of[p.recv_gid[k]] = p.recv_dst[k];
    const int32_t n_local = (int32_t)(T.plane * (size_t)P.nblocks);

    // the operand that stands, at rank R, for interior cell (ig, jg); for other ranks than this one only who owns it matters
    auto operand = [&](int R, int ig, int jg) -> int32_t {
        const HaloBlock *B = T.find(ig, jg);
        if (!B || B->owner < 0) {
            if (X.why.empty())
                X.why = "cell (" + std::to_string(ig) + ", " + std::to_string(jg) + ") that the tripoleT stress symmetrisation of rank " +
                        std::to_string(R) + " reads lies in an eliminated block";
            return -1;
        }
        if (B->owner != R) X.collective = true;
        if (R != T.me) return -1;
        if (B->owner == R) return T.offset(*B, ng + 1 + (ig - B->gi0), ng + 1 + (jg - B->gj0));
        const auto it = slot_of.find((int32_t)((ig - 1) + (size_t)NX * (jg - 1)));
        if (it == slot_of.end() || it->second < n_local || it->second >= n_local + P.cg_tail) {
            if (X.why.empty())
                X.why = "cell (" + std::to_string(ig) + ", " + std::to_string(jg) + ") of rank " + std::to_string(B->owner) +
                        " is not among the fold sources the C grid's exchange carries to rank " + std::to_string(R);
            return -1;
        }
        return it->second;
    };
    for (const HaloBlock &B : T.blk) {
        if (B.owner < 0 || B.gj0 + B.gny - 1 != NY) continue;
        const int R = B.owner;
        const bool mine = R == T.me;
        const int ig_nw = T.wrap(B.gi0 - 1);                // the north-west corner ghost cell
        if (ig_nw != NX / 2 && ig_nw != NX) {
            const int32_t src = operand(R, T.wrap(NX - ig_nw + 2), NY - 1);
            if (mine) { X.corner_dst.push_back(T.offset(B, ng, ng + B.gny + 1)); X.corner_src.push_back(src); }
        }
        const int j = ng + B.gny;
        for (int i = 1; i <= B.gnx + 2 * ng; ++i) {
            const int ig = T.wrap(B.gi0 + (i - ng - 1));
            const int32_t dst = T.offset(B, i, j), src = operand(R, T.wrap(NX - ig + 2), NY);
            if (mine) { X.dst.push_back(dst); X.src.push_back(src); }
            if (i <= ng || i > ng + B.gnx) {              // an east-west ghost cell: image of its own array's cell
                const int32_t own = operand(R, ig, NY);
                if (mine) { X.own_dst.push_back(dst); X.own_src.push_back(own); }
            }
        }
    }
    if (!X.ok()) {
        X.dst.clear(); X.src.clear(); X.own_dst.clear(); X.own_src.clear(); X.corner_dst.clear(); X.corner_src.clear();
    }
}
