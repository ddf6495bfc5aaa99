// =====================================================================
// C ABI of the MI355X-native EVP core (see include/cice_evp_hip.h): life cycle, the
// per-call entry points, the post-loop kernels (f-1, f-3) and introspection.  The device
// state and the helpers live in evp_host*.cpp (overview in evp_host.h).
// =====================================================================
#include "cgrid_schedule.h"
#include "evp_host.h"
#include "rim_plan.h"

using namespace evp_host;

// Read-outs of the plan's lists: v into a caller's int32 list, entry k at out[k * stride]; out may be NULL.  Returns the count.
namespace {
int32_t *at(int32_t *out, size_t k) { return out ? out + k : nullptr; }
template <class T> size_t copy_out(int32_t *out, const std::vector<T> &v, int stride = 1)
{
    for (size_t k = 0; out && k < v.size(); ++k) out[k * stride] = (int32_t)v[k];
    return v.size();
}
// ... one member of every peer, peer after peer
template <class T> size_t copy_out(int32_t *out, const std::vector<HaloPeer> &peers, std::vector<T> HaloPeer::*member, int stride = 1)
{
    size_t n = 0;
    for (const HaloPeer &p : peers) n += copy_out(at(out, n * stride), p.*member, stride);
    return n;
}
}  // namespace

// Every member of the plan built last, in declaration order (halo_plan.h), as int32: a vector as its length and its entries, a
// peer list as its length and every peer member by member, the error text as its length and its characters.  Reads only the struct.
#ifdef CICE_EVP_HIP_TESTING
namespace {
struct PlanDump {
    int32_t *out;
    int32_t n = 0;
    void put(long v) { if (out) out[n] = (int32_t)v; ++n; }
    template <class T> void put(const std::vector<T> &v) { put((long)v.size()); for (const T &x : v) put((long)x); }
    void put(const FoldList &L) { put(L.dst); put(L.a); put(L.b); put(L.flip); }
    void put(const std::vector<HaloPeer> &peers)
    {
        put((long)peers.size());
        for (const HaloPeer &p : peers) {
            put(p.rank); put(p.send_src); put(p.send_dst); put(p.recv_dst); put(p.recv_sign); put(p.recv_gid); put(p.send_sign);
            put(p.n_ghost_send); put(p.n_ghost_recv);
            put(p.fimg_src); put(p.fimg_dst); put(p.fimg_sign); put(p.fimg_recv_dst); put(p.fimg_recv_col); put(p.fimg_recv_sign);
        }
    }
    void put(const HaloPlan &P)
    {
        put(P.nx_block); put(P.ny_block); put(P.nblocks);
        put(P.local_dst); put(P.local_src); put(P.local_sign); put(P.peers);
        put(P.seam_a); put(P.seam_b); put(P.seam_pole); put(P.late_dst); put(P.late_src); put(P.late_sign);
        put(P.fin_dst); put(P.fin_a); put(P.fin_b); put(P.fin_coef); put(P.tail);
        put(P.any_fold_exchange); put(P.stress_remote); put(P.fold_rows);
        put(P.stress_dst); put(P.stress_src); put(P.stress_own_dst); put(P.stress_own_src);
        put(P.stress_corner_dst); put(P.stress_corner_src);
        put(P.center_dst); put(P.center_src); put(P.center_vsign); put(P.tfold);
        put(P.center_tf_dst); put(P.center_tf_a); put(P.center_tf_b); put(P.center_tf_flip);
        put(P.center_tf_remote); put(P.center_remote); put(P.center_fold_remote);
        put(P.center_foldr_dst); put(P.stress_foldr_dst); put(P.fold_shift_cells); put(P.center_seam_dst); put(P.center_seam_slot);
        put(P.fold_split);
        for (const FoldList &L : P.cg_fold) put(L);
        put(P.cg_peers); put(P.cg_tail); put(P.cg_split); put(P.cg_fold_ranks);
        put(std::vector<char>(P.error.begin(), P.error.end()));
    }
};
}  // namespace
#endif

extern "C" {

int cice_evp_hip_abi_version(void) { return CICE_EVP_HIP_ABI_VERSION; }

int cice_evp_hip_last_error(char *buf, int32_t buflen)
{
    if (buf && buflen > 0) {
        std::strncpy(buf, g_err.c_str(), (size_t)buflen - 1);
        buf[buflen - 1] = 0;
    }
    return (int)g_err.size();
}

// host only: the C-grid fold step of one location for the decomposition in `dims` (counts first, then the lists)
#ifdef CICE_EVP_HIP_TESTING
int cice_evp_hip_cgrid_fold_plan(const cice_evp_hip_dims *dims, int32_t loc, int32_t *count, int32_t *dst, int32_t *a,
                                 int32_t *b, int32_t *flip)
{
    if (!dims || !count || loc < 0 || loc > 3) return fail(-1, "bad argument");
    if (dims->ns_boundary_type != CICE_EVP_BND_TRIPOLE && dims->ns_boundary_type != CICE_EVP_BND_TRIPOLET) return fail(-1, "not a tripole grid");
    FoldList L;
    build_fold_list(*dims, loc, L);
    *count = (int32_t)L.dst.size();
    if (dst && a && b && flip)
        for (size_t k = 0; k < L.dst.size(); ++k) { dst[k] = L.dst[k]; a[k] = L.a[k]; b[k] = L.b[k]; flip[k] = L.flip[k]; }
    return 0;
}

int cice_evp_hip_cgrid_window_plan(const cice_evp_hip_dims *dims, int32_t ox, int32_t oy, int32_t *ntiles, int32_t *tiles4, int32_t *tab)
{
    return cice_evp_hip_cgrid_window_plan_ext(dims, ox, oy, 0, ntiles, tiles4, tab);
}

int cice_evp_hip_cgrid_window_plan_ext(const cice_evp_hip_dims *dims, int32_t ox, int32_t oy, int32_t extra, int32_t *ntiles, int32_t *tiles4,
                                       int32_t *tab)
{
    if (!dims || !ntiles || ox < 4 || oy < 4 || extra < 0 || extra > 2) return fail(-1, "bad argument");
    HaloPlan P;
    if (!build_halo_plan(*dims, P)) return fail(-3, "halo plan: %s", P.error.c_str());
    std::vector<int32_t> t4, tb;
    if (extra == 2) {                       // the resident kernel's windows on a tripole grid (17 x 17 positions; ox, oy unused)
        std::vector<int32_t> t2;
        std::string why;
        if (!build_fold_window_table(*dims, P, t4, t2, tb, why)) return fail(-5, "fold windows: %s", why.c_str());
    } else {
        build_window_table(*dims, P, ox, oy, 1 << 20, t4, tb, extra);
    }
    *ntiles = (int32_t)(t4.size() / 4);
    if (tiles4) std::copy(t4.begin(), t4.end(), tiles4);
    if (tab) std::copy(tb.begin(), tb.end(), tab);
    return 0;
}

int cice_evp_hip_cgrid_window_deps(const cice_evp_hip_dims *dims, int32_t *n_windows, int32_t *n_edges, int32_t *n_oneway, int32_t *n_unsafe)
{
    if (!dims || !n_edges || !n_oneway || !n_unsafe) return fail(-1, "bad argument");
    HaloPlan P;
    if (!build_halo_plan(*dims, P)) return fail(-3, "halo plan: %s", P.error.c_str());
    const bool tripole = dims->ns_boundary_type == CICE_EVP_BND_TRIPOLE;
    std::vector<int32_t> t4, t2, tb;
    if (tripole) {
        std::string why;
        if (!build_fold_window_table(*dims, P, t4, t2, tb, why)) return fail(-5, "fold windows: %s", why.c_str());
    } else {
        build_window_table(*dims, P, 16, 16, 1 << 20, t4, tb, 1);
    }
    int ne = 0, n1 = 0;
    *n_unsafe = cgres_dependencies(*dims, tripole, t4, tb, nullptr, &ne, &n1);
    *n_edges = ne;
    *n_oneway = n1;
    if (n_windows) *n_windows = (int32_t)(t4.size() / 4);
    return 0;
}
int cice_evp_hip_cgrid_strip_plan(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t lo0, int32_t slots, int32_t seg_min, int32_t seg,
                                  int32_t *n_items, int32_t *items6, int32_t items_cap, int32_t *n_windows, int32_t *tiles4, uint8_t *in_zone, int32_t windows_cap,
                                  int32_t *seg_rows)
{
    if (!dims || !n_items || !n_windows) return fail(-1, "bad argument");
    HaloPlan P;
    if (!build_halo_plan(*dims, P)) return fail(-3, "halo plan: %s", P.error.c_str());
    std::vector<int32_t> t4, it;
    std::vector<StripZone> zones;
    plan_strip_zones(*dims, P, ex, ey, 62, STRIP_EVERY_IMAGE, t4, zones);
    const int s = strip_items(zones, ex, ey, lo0, slots, seg_min, seg, it);
    std::vector<uint8_t> in;
    strip_windows(zones, t4, in);
    *n_items = (int32_t)(it.size() / 6);
    *n_windows = (int32_t)(t4.size() / 4);
    if (seg_rows) *seg_rows = s;
    if (items6) {
        if ((size_t)items_cap * 6 < it.size()) return fail(-1, "room for %d items, there are %d", items_cap, *n_items);
        std::copy(it.begin(), it.end(), items6);
    }
    if (tiles4 && in_zone) {
        if ((size_t)windows_cap * 4 < t4.size()) return fail(-1, "room for %d windows, there are %d", windows_cap, *n_windows);
        std::copy(t4.begin(), t4.end(), tiles4);
        std::copy(in.begin(), in.end(), in_zone);
    }
    return 0;
}
int cice_evp_hip_cgrid_strip_zones(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t *n_zones, int32_t *zones10, int32_t zones_cap)
{
    if (!dims || !n_zones) return fail(-1, "bad argument");
    HaloPlan P;
    if (!build_halo_plan(*dims, P)) return fail(-3, "halo plan: %s", P.error.c_str());
    std::vector<int32_t> t4;
    std::vector<StripZone> zones;
    plan_strip_zones(*dims, P, ex, ey, 62, STRIP_EVERY_IMAGE, t4, zones);
    *n_zones = (int32_t)zones.size();
    if (!zones10) return 0;
    if ((size_t)zones_cap < zones.size()) return fail(-1, "room for %d rectangles, there are %d", zones_cap, *n_zones);
    for (size_t k = 0; k < zones.size(); ++k) {
        const StripZone &z = zones[k];
        StripRange r;
        const bool ok = strip_len_range(z, ex, ey, dims->nx_block, dims->ny_block, r);
        const int32_t v[10] = {z.b, z.i0, z.i1, z.j0, z.j1, ok ? 1 : 0, r.i0, r.i1, r.j0, r.j1};
        std::copy(v, v + 10, zones10 + 10 * k);
    }
    return 0;
}
int cice_evp_hip_cgrid_frame_plan(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t lo0, int32_t slots, int32_t seg_min, int32_t seg,
                                  int64_t *info6, uint8_t *cells, int32_t *wg, int32_t wg_cap, int32_t *items6, int32_t items_cap)
{
    if (!dims || !info6) return fail(-1, "bad argument");
    HaloPlan P;
    if (!build_halo_plan(*dims, P)) return fail(-3, "halo plan: %s", P.error.c_str());
    std::vector<int32_t> t4, it;
    std::vector<StripZone> zones;
    plan_strip_zones(*dims, P, ex, ey, 62, STRIP_EVERY_IMAGE, t4, zones);
    if (!zones.empty()) strip_items(zones, ex, ey, lo0, slots, seg_min, seg, it);
    CgFramePlan F;
    std::string why;
    const int rc = build_cg_frame(*dims, P, it, F, why);
    if (rc < 0) return fail(-5, "%s", why.c_str());
    for (int k = 0; k < 6; ++k) info6[k] = 0;
    if (rc == 0) return 1;                                    // declined: one rank
    info6[0] = F.zone_cells; info6[1] = F.rest_cells;
    for (int k = 0; k < 3; ++k) info6[2 + k] = (int64_t)F.wg[k].size();
    info6[5] = (int64_t)(it.size() / 6);
    if (cells) std::copy(F.cells.begin(), F.cells.end(), cells);
    if (wg) {
        if ((size_t)wg_cap < F.wg[0].size() + F.wg[1].size() + F.wg[2].size()) return fail(-1, "room for %d workgroups", wg_cap);
        for (int k = 0; k < 3; ++k) wg = std::copy(F.wg[k].begin(), F.wg[k].end(), wg);
    }
    if (items6) {
        if ((size_t)items_cap * 6 < it.size()) return fail(-1, "room for %d items", items_cap);
        std::copy(it.begin(), it.end(), items6);
    }
    return 0;
}
int cice_evp_hip_cgrid_march_fold_plan(const cice_evp_hip_dims *dims, int32_t ex, int32_t ey, int32_t slots, int32_t seg_min, int32_t seg, int32_t len,
                                       int64_t *info11, uint8_t *cells, int32_t *wg, int32_t wg_cap, int32_t *items6, int32_t items_cap,
                                       int32_t ranks, int64_t *ranks3, int32_t *sent, int32_t sent_cap)
{
    if (!dims || !info11) return fail(-1, "bad argument");
    HaloPlan P;
    if (!build_halo_plan(*dims, P)) return fail(-3, "halo plan: %s", P.error.c_str());
    CgMarchFoldPlan F;
    std::string why;
    const int rc = build_cg_march_fold(*dims, P, ex, ey, slots, seg_min, seg, len, nullptr, F, why, ranks != 0);
    if (rc < 0) return fail(-5, "%s", why.c_str());
    for (int k = 0; k < 11; ++k) info11[k] = 0;
    if (ranks3) { ranks3[0] = (int64_t)F.sent.size(); ranks3[1] = F.frame_cells; ranks3[2] = P.cg_split ? P.cg_tail : 0; }
    if (rc == 0) {                                            // declined: the reason is the last error's text
        g_err = why;
        return 1;
    }
    info11[0] = F.zone_cells; info11[1] = F.rest_cells;
    size_t nwg = 0;
    for (int k = 0; k < 5; ++k) { info11[2 + k] = (int64_t)F.wg[k].size(); nwg += F.wg[k].size(); }
    info11[7] = (int64_t)(F.items.size() / 6);
    info11[8] = F.band_rows; info11[9] = F.seg; info11[10] = F.lengths;
    if (cells) std::copy(F.cells.begin(), F.cells.end(), cells);
    if (wg) {
        if ((size_t)wg_cap < nwg) return fail(-1, "room for %d workgroups", wg_cap);
        for (int k = 0; k < 5; ++k) wg = std::copy(F.wg[k].begin(), F.wg[k].end(), wg);
    }
    if (items6) {
        if ((size_t)items_cap * 6 < F.items.size()) return fail(-1, "room for %d items", items_cap);
        std::copy(F.items.begin(), F.items.end(), items6);
    }
    if (sent) {
        if ((size_t)sent_cap < F.sent.size()) return fail(-1, "room for %d sent cells", sent_cap);
        std::copy(F.sent.begin(), F.sent.end(), sent);
    }
    return 0;
}
#endif  // CICE_EVP_HIP_TESTING

int cice_evp_hip_stream_probe(int64_t ncells, double *bytes_per_second)
{
    if (ncells <= 0 || !bytes_per_second) return fail(-1, "bad argument");
    const double sec = evp_stream_probe((size_t)ncells, 5, nullptr);
    if (sec <= 0) return fail((int)-sec, "stream probe failed: %s", hipGetErrorString((hipError_t)(int)-sec));
    *bytes_per_second = 46.0 * 8.0 * (double)ncells / sec;
    return 0;
}

// HIP device of this rank: CICE_EVP_HIP_DEVICE, else the rank's index on its node as the launcher states it
// (torch.distributed.run, Open MPI, MVAPICH2, MPICH / Intel MPI hydra, Slurm), else rank modulo the device count --
// right on one node, and on several when the launcher places ranks block-wise.
static int pick_device(int rank, int ndev)
{
    if (env("CICE_EVP_HIP_DEVICE")) return env_int(env("CICE_EVP_HIP_DEVICE"), 0);
    for (const char *name : {"LOCAL_RANK", "OMPI_COMM_WORLD_LOCAL_RANK", "MV2_COMM_WORLD_LOCAL_RANK", "MPI_LOCALRANKID", "SLURM_LOCALID"})
        if (const char *v = std::getenv(name))
            if (*v >= '0' && *v <= '9') return std::atoi(v) % ndev;
    return rank % ndev;
}

int cice_evp_hip_finalize(void)
{
    if (S.stream) (void)hipStreamSynchronize(S.stream);
    cgrid_free();
    march_free();
    free_all();
    S = State();
    return 0;
}

int cice_evp_hip_init(const cice_evp_hip_dims *dims, const cice_evp_hip_params *params,
                      const double *HTE, const double *HTN, const double *dxT, const double *dyT,
                      const double *uarear, const double *tarea)
{
    if (!dims || !params) return fail(-1, "cice_evp_hip_init: null argument");
    // also after an init that failed midway (S.ready still false): release whatever it had created
    cice_evp_hip_finalize();
    if (dims->nghost != 1) return fail(-1, "nghost must be 1");
    if (dims->nblocks == 0 && dims->nranks > 1) {
        // no blocks on this rank (shared/ice_distribution.F90 hands a task nothing when the processor grid does not divide
        // the block grid): a bystander of the bootstrap, see State::bystander
        S.d = *dims;
        S.d.ilo = S.d.ihi = S.d.jlo = S.d.jhi = S.d.iglob0 = S.d.jglob0 = nullptr;
        S.d.gi0 = S.d.gj0 = S.d.gnx = S.d.gny = S.d.gowner = S.d.glocal = nullptr;
        S.d.nblocks_tot = 0;
        S.prm = *params;
        int ndev = 0;
        HIPC(hipGetDeviceCount(&ndev));
        if (ndev < 1) return fail(-4, "no HIP device");
        S.device = pick_device(dims->rank, ndev);
        HIPC(hipSetDevice(S.device));
        HIPC(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
        S.bystander = true;
        return 0;
    }
    if (!HTE || !HTN || !dxT || !dyT || !uarear || !tarea) return fail(-1, "cice_evp_hip_init: null argument");
    if (dims->nblocks < 1 || dims->nblocks > dims->max_blocks) return fail(-1, "bad nblocks/max_blocks");

    S.d = *dims;
    S.prm = *params;
    const int nb = dims->nblocks;
    S.ilo.assign(dims->ilo, dims->ilo + nb);
    S.ihi.assign(dims->ihi, dims->ihi + nb);
    S.jlo.assign(dims->jlo, dims->jlo + nb);
    S.jhi.assign(dims->jhi, dims->jhi + nb);
    S.iglob0.assign(dims->iglob0, dims->iglob0 + nb);
    S.jglob0.assign(dims->jglob0, dims->jglob0 + nb);
    S.d = host_dims();

    if (!build_halo_plan(*dims, S.plan)) return fail(-3, "halo plan: %s", S.plan.error.c_str());
    build_stress_tfold_xplan(*dims, S.plan, S.stress_x);
    if (env_on(env_test("CICE_EVP_HIP_SELF_EXCHANGE"), false) && dims->nranks == 1) {
        // test hook: route the on-device ghost copies through pack -> ncclSend/ncclRecv (to
        // self) -> unpack, so that the remote-halo code path runs on a single GPU
        HaloPeer self;
        self.rank = dims->rank;
        std::vector<int32_t> kd, ks;
        std::vector<int8_t> kg;
        for (size_t k = 0; k < S.plan.local_dst.size(); ++k) {
            if (S.plan.local_src[k] < 0) {
                kd.push_back(S.plan.local_dst[k]); ks.push_back(-1); kg.push_back(1);
                continue;
            }
            self.send_src.push_back(S.plan.local_src[k]);
            self.send_dst.push_back(S.plan.local_dst[k]);
            self.recv_dst.push_back(S.plan.local_dst[k]);
            self.recv_sign.push_back(S.plan.local_sign[k]);
            self.send_sign.push_back(S.plan.local_sign[k]);
            {
                const int32_t so = S.plan.local_src[k];
                const size_t pl = (size_t)dims->nx_block * dims->ny_block;
                const int b = (int)(so / pl), rem = (int)(so % pl);
                const int j = rem / dims->nx_block + 1, i = rem % dims->nx_block + 1;
                const int ig = dims->iglob0[b] + (i - dims->ilo[b]), jg = dims->jglob0[b] + (j - dims->jlo[b]);
                self.recv_gid.push_back((int32_t)((ig - 1) + (size_t)dims->nx_global * (jg - 1)));
            }
        }
        S.plan.local_dst = kd; S.plan.local_src = ks; S.plan.local_sign = kg;
        self.n_ghost_send = (int)self.send_src.size();
        self.n_ghost_recv = (int)self.recv_dst.size();
        S.plan.peers.push_back(self);
    }
    // the global block table is needed again by plans built later (the marching path decides at the first
    // cice_evp_hip_subcycle): keep a copy -- the caller's arrays need not outlive this call
    {
        const int32_t *src[6] = {dims->gi0, dims->gj0, dims->gnx, dims->gny, dims->gowner, dims->glocal};
        const bool have = dims->nblocks_tot > 0 && src[0] && src[1] && src[2] && src[3] && src[4] && src[5];
        for (int k = 0; k < 6; ++k) {
            S.gtab[k].clear();
            if (have) S.gtab[k].assign(src[k], src[k] + dims->nblocks_tot);
        }
        S.d.gi0 = have ? S.gtab[0].data() : nullptr; S.d.gj0 = have ? S.gtab[1].data() : nullptr;
        S.d.gnx = have ? S.gtab[2].data() : nullptr; S.d.gny = have ? S.gtab[3].data() : nullptr;
        S.d.gowner = have ? S.gtab[4].data() : nullptr; S.d.glocal = have ? S.gtab[5].data() : nullptr;
        if (!have) S.d.nblocks_tot = 0;
    }

    int ndev = 0;
    HIPC(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(-4, "no HIP device");
    const int dev = pick_device(dims->rank, ndev);
    S.device = dev;
    HIPC(hipSetDevice(dev));
    HIPC(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    HIPC(hipStreamCreateWithFlags(&S.stream_comm, hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&S.ev_pack, hipEventDisableTiming));
    HIPC(hipEventCreateWithFlags(&S.ev_halo, hipEventDisableTiming));
    S.overlap = !env_on(env_test("CICE_EVP_HIP_NO_OVERLAP"), false);
    HIPC(hipEventCreate(&S.ev0));
    HIPC(hipEventCreate(&S.ev1));
    HIPC(hipEventCreate(&S.ev2));
    HIPC(hipEventCreate(&S.ev3));
    HIPC(hipEventCreate(&S.evm[0]));
    HIPC(hipEventCreate(&S.evm[1]));

    S.plane = (size_t)dims->nx_block * dims->ny_block;
    S.n = S.plane * nb;
    S.max_ni = S.max_nj = 0;
    std::vector<int4> hb(nb);
    for (int b = 0; b < nb; ++b) {
        hb[b] = make_int4(S.ilo[b], S.ihi[b], S.jlo[b], S.jhi[b]);
        S.max_ni = std::max(S.max_ni, S.ihi[b] - S.ilo[b] + 1);
        S.max_nj = std::max(S.max_nj, S.jhi[b] - S.jlo[b] + 1);
    }
    S.tyb = 4;
    if (const int t = env_int(env_test("CICE_EVP_HIP_TYB"), ENV_UNSET); t != ENV_UNSET) {   // tile height [+100: XCD-contiguous order]
        S.tyb = (t % 100 >= 2 && t % 100 <= 9) ? t : 5 + 100 * (t / 100);
    }
    S.use_graph = !env_on(env_test("CICE_EVP_HIP_NOGRAPH"), false);

    for (auto &p : S.stat)
        if (S.mem.alloc(p, S.n, true)) return -1;
    for (int f = F_STRENGTH; f < F_COUNT; ++f) {
        if (f == F_UVEL || f == F_VVEL) continue;
        if (S.mem.alloc(S.in[f], S.n, true)) return -1;
    }
    S.nuv = S.n + (size_t)S.plan.tail;          // + staging slots for raw seam values of other ranks (tripole, any layout)
    for (int k = 0; k < 2; ++k) {
        if (S.mem.alloc(S.u[k], S.nuv, true) || S.mem.alloc(S.v[k], S.nuv, true)) return -1;
        for (auto &p : S.sig[k])
            if (S.mem.alloc(p, S.n, true)) return -1;
    }
    if (S.mem.alloc(S.hte, S.n, true) || S.mem.alloc(S.htn, S.n, true) || S.mem.alloc(S.vrelfac, S.n, true)) return -1;
    S.flags = EVP_F_VRELFAC;
    S.flags_allowed = ~0u;
    if (env_test("CICE_EVP_HIP_FLAGS")) S.flags_allowed = (unsigned)std::strtoul(env_test("CICE_EVP_HIP_FLAGS"), nullptr, 0);
    if (S.mem.alloc(S.mask, S.n, true) || S.mem.upload(S.blk, hb)) return -1;
    if (upload_lists()) return -1;
    if (build_push_table()) return -1;
    if (S.push_ok) S.flags |= EVP_F_PUSH;
    if (derive_metrics(HTE, HTN, dxT, dyT, uarear, tarea)) return -1;
    S.hmask.resize(S.n);
    S.tyb_forced = env_test("CICE_EVP_HIP_TYB") != nullptr;
    S.ready = true;
    S.uploaded = false;
    S.cur = 0;
    S.fault_calls = 0;
    return 0;
}

int cice_evp_hip_set_metrics(const double *cxp, const double *cyp, const double *cxm,
                             const double *cym, const double *dxhy, const double *dyhx,
                             const double *DminTarea)
{
    if (!S.ready) return fail(-1, "not initialised");
    const double *src[7] = {dxhy, dyhx, cxp, cyp, cxm, cym, DminTarea};   // stat slots 2..8
    for (int k = 0; k < 7; ++k)
        if (src[k] && h2d(S.stat[2 + k], src[k])) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    if (!(S.flags & EVP_F_METRICS)) return 0;      // the kernels read the arrays already
    // The kernels derive the terms from HTE, HTN, dxT, dyT (evp_cell.inc: metrics_cell) and would never look at what was
    // just uploaded: an array that is not that term, bit for bit, on a T-cell a kernel may evaluate (every block's
    // ilo .. ihi+1 x jlo .. jhi+1) takes the shortcut away -- dxhy / dyhx alone keep the other five derived.
    std::vector<double> hte(S.n), htn(S.n), dxT(S.n), dyT(S.n);
    const size_t bytes = S.n * sizeof(double);
    HIPC(hipMemcpy(hte.data(), S.hte, bytes, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(htn.data(), S.htn, bytes, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(dxT.data(), S.stat[0], bytes, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(dyT.data(), S.stat[1], bytes, hipMemcpyDeviceToHost));
    const int nx = S.d.nx_block;
    const double p5 = 0.5, c1p5 = 1.5, dmin = S.prm.deltaminEVP;
    bool differs[7] = {};
    for (int k = 0; k < 7; ++k) {
        if (!src[k]) continue;
        for (int b = 0; b < S.d.nblocks && !differs[k]; ++b)
            for (int j = S.jlo[b]; j <= S.jhi[b] + 1 && !differs[k]; ++j)
                for (int i = S.ilo[b]; i <= S.ihi[b] + 1; ++i) {
                    // (column ihi+1 / row jhi+1 of a block at a boundary that is not cyclic lies outside the domain: no ice there,
                    // and the host model's halo update leaves another value there than the local difference)
                    const int ig = S.iglob0[b] + (i - S.ilo[b]), jg = S.jglob0[b] + (j - S.jlo[b]);
                    if ((ig > S.d.nx_global && S.d.ew_boundary_type != CICE_EVP_BND_CYCLIC) ||
                        (jg > S.d.ny_global && S.d.ns_boundary_type != CICE_EVP_BND_CYCLIC)) continue;
                    const size_t c = (size_t)b * S.plane + (size_t)(j - 1) * nx + (i - 1);
                    double e;
                    switch (k) {
                    case 0: e = p5 * (hte[c] - hte[c - 1]); break;
                    case 1: e = p5 * (htn[c] - htn[c - nx]); break;
                    case 2: e = (c1p5 * htn[c] - p5 * htn[c - nx]); break;
                    case 3: e = (c1p5 * hte[c] - p5 * hte[c - 1]); break;
                    case 4: e = -(c1p5 * htn[c - nx] - p5 * htn[c]); break;
                    case 5: e = -(c1p5 * hte[c - 1] - p5 * hte[c]); break;
                    default: { const double tarea = dxT[c] * dyT[c]; e = dmin * tarea; }
                    }
                    if (std::memcmp(&e, &src[k][c], 8) != 0) { differs[k] = true; break; }
                }
    }
    if (differs[2] || differs[3] || differs[4] || differs[5] || differs[6]) S.flags &= ~EVP_F_METRICS;
    else if (differs[0] || differs[1]) S.flags |= EVP_F_DXHY_ARRAY;
    return 0;
}

static int upload_impl(const double *const *f, const int32_t *iceTmask, const int32_t *iceUmask, bool keep_sig)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (!f || !iceTmask || !iceUmask) return fail(-1, "null argument");
    // (every argument check comes before the first copy is enqueued)
    if (!f[F_WATERX] || !f[F_WATERY] || !f[F_TBU]) return fail(-1, "null field (waterxU / wateryU / TbU)");
    HIPC(hipEventRecord(S.ev2, S.stream));
    CopyBatch B;
    if (!keep_sig) {
        S.cur = 0;
        for (int k = 0; k < 12; ++k) {
            if (!f[k]) return fail(-1, "null stress field %d", k);
            B.items.push_back({S.sig[0][k], f[k]});
        }
    }
    const int cur = S.cur;      // keep_sig: the stresses of the previous call live in sig[cur]
    for (int fi = F_STRENGTH; fi < F_COUNT; ++fi) {
        if (fi == F_UVEL || fi == F_VVEL) continue;
        if ((fi == F_UVEL_INIT || fi == F_VVEL_INIT) && (!f[fi] || S.prm.revp == 0.0)) continue;   // only read when revp = 1
        if (fi == F_WATERX || fi == F_WATERY || fi == F_TBU) continue;   // below: only where the kernels will read them
        // lean call (cice_evp_hip_run on page-locked arrays): the loop writes these four on ice U-cells only and the
        // download writes back those cells only, so the caller's values elsewhere never need to travel
        if (S.lean_diag && (fi == F_STRINTX || fi == F_STRINTY || fi == F_TAUBX || fi == F_TAUBY)) continue;
        // (strintx/y, taubx/y are outputs of the loop on ice U-cells only; elsewhere the caller's values -- zeroed by
        // dyn_prep2 -- must survive the download, so they travel in as well)
        if (!f[fi]) return fail(-1, "null field %d", fi);
        B.items.push_back({S.in[fi], f[fi]});
    }
    if (S.prm.revp != 0.0 && (!f[F_UVEL_INIT] || !f[F_VVEL_INIT]))
        return fail(-1, "uvel_init/vvel_init required for revised EVP");
    if (!f[F_UVEL] || !f[F_VVEL]) return fail(-1, "null velocity field");
    B.items.push_back({S.u[cur], f[F_UVEL]});
    B.items.push_back({S.v[cur], f[F_VVEL]});
    if (h2d_batch(B)) return -1;
    {   // the second ping-pong copy of what was uploaded: one launch
        EvpCopyTab T{};
        T.len = S.n;
        T.vec2 = 1;
        if (!keep_sig)
            for (int k = 0; k < 12; ++k) { T.src[T.n] = S.sig[0][k]; T.dst[T.n] = S.sig[1][k]; ++T.n; }
        T.src[T.n] = S.u[cur]; T.dst[T.n] = S.u[cur ^ 1]; ++T.n;
        T.src[T.n] = S.v[cur]; T.dst[T.n] = S.v[cur ^ 1]; ++T.n;
        for (int k = 0; k < T.n; ++k)
            if ((((uintptr_t)T.src[k]) | ((uintptr_t)T.dst[k])) & 15u) T.vec2 = 0;
        evp_launch_copy_many(T, S.stream);
    }
    // While that batch travels the host scans the caller's arrays for what the kernels will not read in this call:
    // waterx / watery where they equal uocn / vocn bit for bit on every ice U-cell, TbU where it is zero there (with
    // uvel_init / vvel_init under classic EVP: five of the 32 arrays of the default configuration stay on the host).
    bool water_is_ocn = true, tbu_zero = true;
    {
        const double *wx = f[F_WATERX], *wy = f[F_WATERY], *uo = f[F_UOCN], *vo = f[F_VOCN], *tb = f[F_TBU];
        const double plus0 = 0.0;
        for (size_t k = 0; k < S.n; ++k) S.hmask[k] = (uint8_t)((iceTmask[k] != 0 ? 1 : 0) | (iceUmask[k] != 0 ? 2 : 0));
        // (the U-cells a kernel advances: iceUmask on the physical cells of each block.  A caller may hold iceUmask on ghost cells
        // too -- images of cells another block or rank advances, and judges)
        const int nxb = S.d.nx_block;
        for (int b = 0; b < S.d.nblocks; ++b)
            for (int j = S.jlo[b]; j <= S.jhi[b]; ++j)
                for (int i = S.ilo[b]; i <= S.ihi[b]; ++i) {
                    const size_t k = (size_t)b * S.plane + (size_t)(j - 1) * nxb + (i - 1);
                    if (!(S.hmask[k] & 2u)) continue;
                    // bit-for-bit identical operands (cosw=1, sinw=0: ice_dyn_shared.F90:69-70,819-820)
                    if (std::memcmp(&wx[k], &uo[k], 8) != 0 || std::memcmp(&wy[k], &vo[k], 8) != 0) water_is_ocn = false;
                    // (bits: TbU = -0.0 gives Cb = -0.0 and taubx = -uvel*Cb the other sign of zero, :939, 964-965)
                    if (std::memcmp(&tb[k], &plus0, 8) != 0) tbu_zero = false;
                }
        CopyBatch B2;
        if (!(water_is_ocn && (S.flags_allowed & EVP_F_WATER_IS_OCN))) {
            B2.items.push_back({S.in[F_WATERX], wx});
            B2.items.push_back({S.in[F_WATERY], wy});
        }
        if (!(tbu_zero && (S.flags_allowed & EVP_F_TBU_ZERO))) B2.items.push_back({S.in[F_TBU], tb});
        if (!B2.items.empty() && h2d_batch(B2)) return -1;
    }
    if (S.lean_diag) {
        // bit 7: the cells the loop really writes strintx/y, taubx/y on -- iceUmask on INTERIOR cells.  A caller may
        // hold iceUmask on ghost or padding cells too (halo-updated masks): the masked scatter of the download must
        // not hand never-written device values back there.  Kernels test bits 0 and 1 only.
        const int nxb = S.d.nx_block;
        for (int b = 0; b < S.d.nblocks; ++b)
            for (int j = S.d.jlo[b]; j <= S.d.jhi[b]; ++j)
                for (int i = S.d.ilo[b]; i <= S.d.ihi[b]; ++i) {
                    const size_t k = (size_t)b * S.plane + (size_t)(j - 1) * nxb + (i - 1);
                    if (S.hmask[k] & 2u) S.hmask[k] |= 0x80u;
                }
    }
    S.flags &= ~(EVP_F_WATER_IS_OCN | EVP_F_TBU_ZERO);
    if (water_is_ocn) S.flags |= EVP_F_WATER_IS_OCN;
    if (tbu_zero) S.flags |= EVP_F_TBU_ZERO;
    evp_launch_vrelfac(S.in[F_AIX], S.in[F_CW], S.prm.rhow, S.vrelfac, S.n, S.stream);
    HIPC(hipMemcpyAsync(S.mask, S.hmask.data(), S.n, hipMemcpyHostToDevice, S.stream));
    if (keep_sig) evp_launch_zero_sig_off_mask(S.sig[0], S.sig[1], S.mask, S.n, S.stream);
    HIPC(hipEventRecord(S.ev3, S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, S.ev2, S.ev3));
    S.t_h2d_ms = ms;
    S.uploaded = true;
    ++S.upload_seq;
    if (S.hmask_prev != S.hmask) { S.res2_order_stale = true; S.hmask_prev = S.hmask; }
    return tune_after_upload();
}

int cice_evp_hip_upload(const double *const *f, const int32_t *iceTmask, const int32_t *iceUmask)
{
    S.sig_valid = false;
    return upload_impl(f, iceTmask, iceUmask, false);
}

int cice_evp_hip_subcycle(int32_t ndte)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    if (ndte < 0) return fail(-1, "ndte < 0");
    if (ndte == 0) return 0;
    HIPC(hipEventRecord(S.ev0, S.stream));
    // (the tiles that hold ice must all be on the chip at once: checked against THIS call's masks -- a call with more ice than that
    // goes through the kernels below, the next one is asked again)
    S.res_ran = S.res_mode == 1 && !resident_declined_switch() && resident2_fits_now();
    if (S.res_ran) {
        if (int rc = launch_resident2(ndte, S.cur, false)) return rc;
        S.res_launched = true;
        HIPC(hipEventRecord(S.ev1, S.stream));
        S.cur ^= (ndte & 1);
        S.t_nsub = ndte;
        return 0;
    }
    S.march.last_call = false;
    if (march_wanted()) {
        // large per-rank domain: several subcycles per pass over HBM (evp_march.hip); falls back to the loop below by
        // itself when the uploaded state does not qualify
        const int declined0 = S.march.declined;
        if (int rc = march_run(ndte)) return rc;
        S.march.last_call = S.march.declined == declined0;
        HIPC(hipEventRecord(S.ev1, S.stream));
        S.t_nsub = ndte;
        return 0;
    }
    // RCCL p2p inside a captured graph: opt-in (CICE_EVP_HIP_GRAPH_RCCL=1) until measured on a multi-GPU node
    const bool graph_rccl = env_on(env_test("CICE_EVP_HIP_GRAPH_RCCL"), false);
    const bool graph_ok = S.use_graph && (S.plan.peers.empty() || graph_rccl || S.direct.on);
    if (graph_ok) {
        const auto key = std::make_tuple((int)ndte, S.cur, S.flags & S.flags_allowed);
        auto it = S.graphs.find(key);
        if (it == S.graphs.end()) {
            hipGraph_t g = nullptr;
            hipGraphExec_t ge = nullptr;
            if (use_overlap() || use_riding_exchange()) {   // device allocations are not allowed while capturing
                State::TileSplit *ts = nullptr;
                if (int rc = get_tile_split(S.tyb % 100, &ts)) return rc;
            }
            HIPC(hipStreamBeginCapture(S.stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue_loop(ndte, S.cur);
            hipError_t e = hipStreamEndCapture(S.stream, &g);
            if (rc) return rc;
            if (e != hipSuccess) return fail((int)e, "hipStreamEndCapture: %s", hipGetErrorString(e));
            HIPC(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
            HIPC(hipGraphDestroy(g));
            it = S.graphs.emplace(key, ge).first;
            // the event recorded before the capture is stale for timing; re-record
            HIPC(hipEventRecord(S.ev0, S.stream));
        }
        HIPC(hipGraphLaunch(it->second, S.stream));
    } else {
        if (int rc = enqueue_loop(ndte, S.cur)) return rc;
    }
    HIPC(hipEventRecord(S.ev1, S.stream));
    S.cur ^= (ndte & 1);
    S.t_nsub = ndte;
    return 0;
}

// tripoleT with a top-row partner on another rank: the symmetrisation goes through the fold exchange (S.stress_x; the same
// answer on every rank, the exchange is a collective)
static bool stress_tfold_exchange() { return S.plan.tfold && S.stress_x.ok() && S.stress_x.collective; }

// 1 if cice_evp_hip_stress_halo can do its job on this rank layout (tripole: always; tripoleT: no eliminated block among the
// cells the top row mirrors; other boundaries: there is nothing to do, 1), else 0 -- for a host that wants to keep the stresses
// on the device between calls and must know whether evp()'s twelve ice_HaloUpdate_stress calls can be left to the library.
int cice_evp_hip_stress_halo_available(void)
{
    if (!S.ready) return 0;
    if (stress_tfold_exchange()) return 1;
    return (S.plan.tfold && S.plan.stress_remote) ? 0 : 1;
}

// Tripole: force the stresses symmetric across the seam on the resident state, as evp() does
// on the host arrays after the subcycle loop (12 x ice_HaloUpdate_stress, ice_dyn_evp.F90:1321-1389).
int cice_evp_hip_stress_halo(void)
{
    if (!S.ready) return fail(-1, "state not uploaded");
    // (the layout's verdict first: it does not depend on what has been uploaded)
    if (S.plan.tfold && S.plan.stress_remote && !stress_tfold_exchange())
        return fail(-9, "tripoleT: on this layout the stress symmetrisation stays with the host (evp() applies it to its own "
                        "arrays, ice_dyn_evp.F90:1321-1389): %s", S.stress_x.why.c_str());
    if (!S.uploaded) return fail(-1, "state not uploaded");
    if (S.plan.tfold) {
        // the top row on several ranks: each pair (a1, a2) through the C grid's fold exchange, then the three lists with the
        // partners' values in staging slots -- collective, as the u-fold form below
        if (stress_tfold_exchange()) return stress_tfold_split();
        evp_launch_halo_stress_tfold(S.sig[S.cur], S.h_stress_dst, S.h_stress_src, S.n_stress, S.h_stress_own_dst, S.h_stress_own_src,
                                     S.n_stress_own, S.stream);
        // the north-west corner ghost cells: both arrays of a pair, each from the other's row NY-1 (which nothing above writes)
        evp_launch_halo_stress(S.sig[S.cur], S.h_stress_corner_dst, S.h_stress_corner_src, S.n_stress_corner, S.stream);
        HIPC(hipGetLastError());
        return 0;
    }
    evp_launch_halo_stress(S.sig[S.cur], S.h_stress_dst, S.h_stress_src, S.n_stress, S.stream);
    // partners on other ranks (fold row split in x): a1's ghost row <- a2's top row through the exchange of a shifted copy
    // (halo_plan.h); collective -- a rank without destinations of its own still serves its top row.  Scalars: factor -1.
    if (S.plan.fold_split)
        for (int fam = 0; fam < 12; fam += 4)
            for (int q = fam; q < fam + 2; ++q) {
                double *a1 = S.sig[S.cur][q], *a2 = S.sig[S.cur][q ^ 2];
                if (int rc = fold_remote_pair(a2, a1, a1, a2, 1, -1.0, -1.0)) return rc;
            }
    HIPC(hipGetLastError());
    return 0;
}


// Record a HIP event on the library's stream: which = 0 (begin) or 1 (end) of a caller's
// timed region; the elapsed time is reported by cice_evp_hip_get_timings()[6].
int cice_evp_hip_mark(int32_t which)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (which < 0 || which > 1) return fail(-1, "mark index");
    HIPC(hipEventRecord(S.evm[which], S.stream));
    S.marked[which] = true;
    return 0;
}

// ---- next tier: deformations and dyn_finish on the resident final state ----
int cice_evp_hip_set_post_geometry(const double *dxU, const double *dyU, const double *tarear)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (!dxU || !dyU || !tarear) return fail(-1, "null argument");
    const double *src[3] = {dxU, dyU, tarear};
    for (int k = 0; k < 3; ++k) {
        if (!S.post_geo[k] && S.mem.alloc(S.post_geo[k], S.n, true)) return -1;
        if (h2d(S.post_geo[k], src[k])) return -1;
    }
    for (auto &p : S.post_out)
        if (!p && S.mem.alloc(p, S.n, true)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    S.have_post_geo = true;
    return 0;
}

int cice_evp_hip_deformations(double *divu, double *shear, double *vort, double *rdg_conv, double *rdg_shear)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    if (!S.have_post_geo) return fail(-1, "cice_evp_hip_set_post_geometry not called");
    EvpArgs A;
    fill_args(A, S.cur, 0);
    evp_launch_deformations(A, S.d.nblocks, S.prm.strict != 0, S.post_geo[0], S.post_geo[1], S.post_geo[2],
                            S.post_out[0], S.post_out[1], S.post_out[2], S.post_out[3], S.post_out[4], S.stream);
    double *dst[5] = {divu, shear, vort, rdg_conv, rdg_shear};
    for (int k = 0; k < 5; ++k)
        if (dst[k] && d2h(dst[k], S.post_out[k])) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

int cice_evp_hip_dyn_finish(double *strocnxU, double *strocnyU)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    if (!strocnxU || !strocnyU) return fail(-1, "null argument");
    for (int k = 5; k < 7; ++k)
        if (!S.post_out[k] && S.mem.alloc(S.post_out[k], S.n, true)) return -1;
    // inout: cells outside the ice keep the caller's values (dyn_prep2 zeroes them, :776-784)
    if (h2d(S.post_out[5], strocnxU) || h2d(S.post_out[6], strocnyU)) return -1;
    EvpArgs A;
    fill_args(A, S.cur, 0);
    evp_launch_dyn_finish(A, S.d.nblocks, S.prm.strict != 0, S.post_out[5], S.post_out[6], S.stream);
    if (d2h(strocnxU, S.post_out[5]) || d2h(strocnyU, S.post_out[6])) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    S.tail.strocn = true;              // the device copy stays: cice_evp_hip_strocn_t reads it
    S.tail.strocn_seq = S.upload_seq;
    return 0;
}

// Page-lock a caller-owned host array so that the H2D/D2H copies of cice_evp_hip_run become
// direct DMA (pageable copies of gx1's 50 arrays cost ~14 ms per call, pinned ~1.5 ms).  For
// arrays that live as long as the library is initialised -- CICE's module arrays.  Idempotent;
// unregistered by cice_evp_hip_finalize.
int cice_evp_hip_pin_host(const void *ptr, int64_t bytes)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (!ptr || bytes <= 0) return fail(-1, "bad argument");
    auto it = S.pinned.find(ptr);
    if (it != S.pinned.end() && it->second.bytes >= (size_t)bytes) return 0;
    if (it != S.pinned.end()) {
        (void)hipHostUnregister(const_cast<void *>(ptr));
        S.pinned.erase(it);
    }
    // mapped: the device can address the range itself, so the per-call traffic becomes one gather and one
    // scatter launch (evp_copy.hip) instead of one copy per array
    void *dev = nullptr;
    if (hipHostRegister(const_cast<void *>(ptr), (size_t)bytes, hipHostRegisterMapped) == hipSuccess) {
        if (hipHostGetDevicePointer(&dev, const_cast<void *>(ptr), 0) != hipSuccess) dev = nullptr;
    } else {
        (void)hipGetLastError();
        HIPC(hipHostRegister(const_cast<void *>(ptr), (size_t)bytes, hipHostRegisterDefault));
    }
    S.pinned[ptr] = State::Pinned{(size_t)bytes, dev};
    return 0;
}

// Options of the per-call entry points.  CICE_EVP_HIP_OPT_STRESS_RESIDENT (1): the 12 stress components
// stay on the device between calls of cice_evp_hip_run -- evp() is their only writer (ice_dyn_evp.F90), so
// they are uploaded on the first call only (and after cice_evp_hip_invalidate_stresses), zeroed off
// iceTmask on the device as dyn_prep2 does on the host, and not downloaded; the caller fetches them when
// something else needs them (restart / history: cice_evp_hip_fetch_stresses).
int cice_evp_hip_set_option(int32_t key, int32_t value)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (key == CICE_EVP_HIP_OPT_STRESS_RESIDENT) {
        S.opt_sig_resident = value != 0;
        if (!S.opt_sig_resident) S.sig_valid = false;
        return 0;
    }
    return fail(-1, "unknown option %d", (int)key);
}

int cice_evp_hip_invalidate_stresses(void)
{
    S.sig_valid = false;
    return 0;
}

int cice_evp_hip_fetch_stresses(double *const *sig12)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    if (!sig12) return fail(-1, "null argument");
    HIPC(hipStreamSynchronize(S.stream));
    if (int rc = resident_check_error()) return rc;
    CopyBatch B;
    for (int k = 0; k < 12; ++k)
        if (sig12[k]) B.items.push_back({sig12[k], S.sig[S.cur][k]});
    if (d2h_batch(B)) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

int cice_evp_hip_sync(void)
{
    if (!S.ready) return fail(-1, "not initialised");
    HIPC(hipStreamSynchronize(S.stream));
    if (int rc = direct_check_error()) return rc;
    if (int rc = march_direct_error()) return rc;
    return resident_check_error();
}

int cice_evp_hip_download(double *const *f)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    HIPC(hipStreamSynchronize(S.stream));
    if (int rc = direct_check_error()) return rc;
    if (int rc = march_direct_error()) return rc;
    if (int rc = resident_check_error()) return rc;
    HIPC(hipEventRecord(S.ev2, S.stream));
    CopyBatch B;
    for (int k = 0; k < 12; ++k)
        if (f[k]) B.items.push_back({f[k], S.sig[S.cur][k]});
    const int outs[4] = {F_STRINTX, F_STRINTY, F_TAUBX, F_TAUBY};
    if (S.lean_diag) {
        CopyBatch M;
        for (int o : outs)
            if (f[o]) M.items.push_back({f[o], S.in[o]});
        if (d2h_batch_masked(M, 0x80u)) return -1;          // bit7: interior && iceUmask = the cells the loop wrote
    } else {
        for (int o : outs)
            if (f[o]) B.items.push_back({f[o], S.in[o]});
    }
    if (f[F_UVEL]) B.items.push_back({f[F_UVEL], S.u[S.cur]});
    if (f[F_VVEL]) B.items.push_back({f[F_VVEL], S.v[S.cur]});
    if (d2h_batch(B)) return -1;
    HIPC(hipEventRecord(S.ev3, S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, S.ev2, S.ev3));
    S.t_d2h_ms = ms;
    if (S.t_nsub > 0 && hipEventElapsedTime(&ms, S.ev0, S.ev1) == hipSuccess) S.t_loop_ms = ms;
    return 0;
}

// Test hook: the N-th call that reaches it reports a failure that did not happen (N = value of the variable), so
// that recovery paths can be exercised on a healthy GPU.
static bool fault_hook(const char *name)
{
    const char *e = env_test(name);
    return e && ++S.fault_calls == std::atoi(e);      // counted from cice_evp_hip_init
}

int cice_evp_hip_run(double *stressp_1, double *stressp_2, double *stressp_3, double *stressp_4,
                     double *stressm_1, double *stressm_2, double *stressm_3, double *stressm_4,
                     double *stress12_1, double *stress12_2, double *stress12_3, double *stress12_4,
                     const double *strength, const double *cdn_ocnU, const double *aiU,
                     const double *uocnU, const double *vocnU, const double *waterxU,
                     const double *wateryU, const double *forcexU, const double *forceyU,
                     const double *umassdti, const double *fmU, double *strintxU, double *strintyU,
                     const double *TbU, double *taubxU, double *taubyU, double *uvel, double *vvel,
                     const double *uvel_init, const double *vvel_init, const int32_t *iceTmask,
                     const int32_t *iceUmask, int32_t ndte)
{
    double *f[F_COUNT] = {stressp_1, stressp_2, stressp_3, stressp_4, stressm_1, stressm_2,
                          stressm_3, stressm_4, stress12_1, stress12_2, stress12_3, stress12_4,
                          (double *)strength, (double *)cdn_ocnU, (double *)aiU, (double *)uocnU,
                          (double *)vocnU, (double *)waterxU, (double *)wateryU, (double *)forcexU,
                          (double *)forceyU, (double *)umassdti, (double *)fmU, strintxU, strintyU,
                          (double *)TbU, taubxU, taubyU, uvel, vvel, (double *)uvel_init,
                          (double *)vvel_init};
    // stresses that never left the device (CICE_EVP_HIP_OPT_STRESS_RESIDENT): no upload, dyn_prep2's zeroing on the device
    const bool keep_sig = S.opt_sig_resident && S.sig_valid && S.uploaded;
    {
        CopyBatch D;
        for (double *p : {strintxU, strintyU, taubxU, taubyU})
            if (p) D.items.push_back({p, nullptr});
        S.lean_diag = D.items.size() == 4 && batch_mapped(D, false) &&
                      env_on(env_test("CICE_EVP_HIP_LEAN"), true);
    }
    struct LeanOff { ~LeanOff() { S.lean_diag = false; } } lean_off;      // only for the duration of this call
    if (int rc = upload_impl(f, iceTmask, iceUmask, keep_sig)) return rc;
    // The resident kernel assumes the GPU to itself.  If that did not hold (another process or a long kernel on the
    // device: a wait gave up) the call is repeated with the streaming kernel, which is then kept.  Without resident
    // stresses nothing has been written back yet and the caller's inputs are intact.  With them (keep_sig) the only
    // copy of the pre-call stresses is sig[cur], which the resident kernel overwrites at its end when ndte is even (it
    // stores into sig[cur ^ (ndte & 1)]; the general variants into both ping-pong copies): keep a device snapshot for the replay.
    const bool may_replay = S.res_mode == 1 && S.plan.peers.empty();
    const int cur0 = S.cur;
    if (may_replay && keep_sig) {
        EvpCopyTab T{};
        T.len = S.n;
        T.vec2 = 1;
        for (int k = 0; k < 12; ++k) {
            if (!S.sig_snap[k])
                if (int rc = S.mem.alloc(S.sig_snap[k], S.n)) return rc;
            T.src[T.n] = S.sig[cur0][k]; T.dst[T.n] = S.sig_snap[k]; ++T.n;
            if ((((uintptr_t)T.src[k]) | ((uintptr_t)T.dst[k])) & 15u) T.vec2 = 0;
        }
        evp_launch_copy_many(T, S.stream);
    }
    S.sig_valid = false;                      // until this call has succeeded
    if (int rc = cice_evp_hip_subcycle(ndte)) return rc;
    if (may_replay) {
        HIPC(hipStreamSynchronize(S.stream));
        if (resident_check_error() != 0 || fault_hook("CICE_EVP_HIP_FAULT_REPLAY")) {
            if (env("CICE_EVP_HIP_VERBOSE"))
                std::fprintf(stderr, "[cice_evp_hip] %s -- repeating the call with the streaming kernel\n", g_err.c_str());
            g_err.clear();
            ++S.res_fallbacks;
            S.res_mode = 0;
            if (keep_sig) {
                EvpCopyTab T{};
                T.len = S.n;
                T.vec2 = 1;
                for (int k = 0; k < 12; ++k) {
                    T.src[T.n] = S.sig_snap[k]; T.dst[T.n] = S.sig[cur0][k]; ++T.n;
                    if ((((uintptr_t)T.src[k]) | ((uintptr_t)T.dst[k])) & 15u) T.vec2 = 0;
                }
                evp_launch_copy_many(T, S.stream);
                S.cur = cur0;
            }
            if (int rc = upload_impl(f, iceTmask, iceUmask, keep_sig)) return rc;
            if (int rc = cice_evp_hip_subcycle(ndte)) return rc;
            // the resident kernel is off from here on (res_mode = 0): the snapshot has no further use
            HIPC(hipStreamSynchronize(S.stream));
            for (auto &q : S.sig_snap) S.mem.free_one(q);
        }
    }
    // only the documented outputs travel back
    double *o[F_COUNT] = {};
    if (!S.opt_sig_resident)
        for (int k = 0; k < 12; ++k) o[k] = f[k];
    o[F_STRINTX] = strintxU; o[F_STRINTY] = strintyU; o[F_TAUBX] = taubxU; o[F_TAUBY] = taubyU;
    o[F_UVEL] = uvel; o[F_VVEL] = vvel;
    if (int rc = cice_evp_hip_download(o)) return rc;          // incl. the error words of the kernels
    S.sig_valid = S.opt_sig_resident;                          // only a call that succeeded leaves valid resident stresses
    return 0;
}

int cice_evp_hip_get_timings(double *out, int32_t n)
{
    float ms = 0;
    if (S.ready && S.t_nsub > 0 && hipEventQuery(S.ev1) == hipSuccess &&
        hipEventElapsedTime(&ms, S.ev0, S.ev1) == hipSuccess)
        S.t_loop_ms = ms;
    double marks_ms = -1.0;
    if (S.ready && S.marked[0] && S.marked[1] && hipEventQuery(S.evm[1]) == hipSuccess &&
        hipEventElapsedTime(&ms, S.evm[0], S.evm[1]) == hipSuccess)
        marks_ms = ms;
    const bool res = S.res_mode == 1 && S.res_ran;
    const double v[16] = {S.t_loop_ms, S.t_h2d_ms, S.t_d2h_ms, (double)S.t_nsub,
                         res ? 1.0 / std::max(S.t_nsub, 1) : S.march.last_call ? (double)S.march.call_passes / std::max(S.march.call_subcycles, 1) :
                         1.0 + ((S.n_local > 0 && !(S.push_ok && (S.flags & S.flags_allowed & EVP_F_PUSH))) ? 1.0 : 0.0) +
                             (S.plan.peers.empty() ? 0.0 : (S.direct.on ? (use_riding_exchange() ? 0.0 : 1.0) : 2.0)) + ((S.n_seam + S.n_pole + S.n_late) > 0 ? 1.0 : 0.0),
                         (double)(res ? 2000 + S.res2_logw : (S.march.last_call ? 3000 + S.march.L.seglen : S.tyb)), marks_ms, S.t_stream_probe_ms, S.t_res_probe_ms,
                          S.plan.peers.empty() ? 0.0 : (S.direct.on ? 2.0 : 1.0), S.prep.t_ms, (double)S.res_fallbacks,
                          (double)(S.msk.on ? S.msk.n_send : S.n_send), (double)(S.msk.on ? S.msk.n_recv : S.n_recv),
                          (double)(res ? (S.res2_nlive > 0 ? S.res2_nlive : S.res2_ntiles) : 0), (double)(S.res_mode == 1 ? S.res2_ntiles : 0)};
    for (int k = 0; k < n && k < 16; ++k) out[k] = v[k];
    return 0;
}

// Per-launch durations of the two kernels of a subcycle, measured with HIP events
// on the library's own stream (the stream the kernels are launched on).  Works on
// the resident state without advancing it: the launches write the ping-pong
// "next" buffers, which the next real subcycle overwrites anyway.
int cice_evp_hip_time_kernels(int32_t nrep, double *out3)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    if (nrep < 1) nrep = 1;
    std::vector<hipEvent_t> ev(2 * (size_t)nrep + 2);
    for (auto &e : ev) HIPC(hipEventCreate(&e));
    const bool strict = S.prm.strict != 0;
    const int cap = cap_mode();
    EvpArgs A;
    fill_args(A, S.cur, 0);
    double sum[2] = {0, 0};
    for (int which = 0; which < 2; ++which) {
        for (int r = 0; r < nrep; ++r) {
            HIPC(hipEventRecord(ev[2 * r], S.stream));
            if (which == 0) evp_launch_subcycle(A, S.max_ni, S.max_nj, S.d.nblocks, S.tyb, strict, cap, S.stream);
            else evp_launch_halo_local(S.u[S.cur ^ 1], S.v[S.cur ^ 1], S.h_local_dst, S.h_local_src,
                                       (const signed char *)S.h_local_sign, S.n_local, S.stream);
            HIPC(hipEventRecord(ev[2 * r + 1], S.stream));
        }
        HIPC(hipStreamSynchronize(S.stream));
        for (int r = 0; r < nrep; ++r) {
            float ms = 0;
            HIPC(hipEventElapsedTime(&ms, ev[2 * r], ev[2 * r + 1]));
            sum[which] += ms;
        }
    }
    // back-to-back period of the stencil kernel (launch gap included)
    HIPC(hipEventRecord(ev[2 * nrep], S.stream));
    for (int r = 0; r < nrep; ++r)
        evp_launch_subcycle(A, S.max_ni, S.max_nj, S.d.nblocks, S.tyb, strict, cap, S.stream);
    HIPC(hipEventRecord(ev[2 * nrep + 1], S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    float ms = 0;
    HIPC(hipEventElapsedTime(&ms, ev[2 * nrep], ev[2 * nrep + 1]));
    out3[0] = sum[0] / nrep;
    out3[1] = S.n_local > 0 ? sum[1] / nrep : 0.0;
    out3[2] = ms / nrep;
    for (auto &e : ev) (void)hipEventDestroy(e);
    return 0;
}

#ifdef CICE_EVP_HIP_TESTING
int cice_evp_hip_debug_device_allocs(int64_t *count)
{
    if (!count) return fail(-1, "null argument");
    *count = (int64_t)(S.mem.owned.size() + march_allocs() + cgrid_allocs());
    return 0;
}

// Per-CU record of the last resident launch (16 x 16 tiles): 2048 CUs x {lock, stamp, ice-holding waves
// on SIMD 0..3, 0, 0}; for tools that check how evenly the workgroups spread their waves.
int cice_evp_hip_debug_cuload(int32_t *out, int32_t n)
{
    if (!S.ready) return fail(-1, "not initialised");
    if (!S.res2_cuload) return fail(-1, "no resident launch with 16 x 16 tiles yet");
    if (!out || n < 0 || n > 2048 * 8) return fail(-1, "bad argument");
    HIPC(hipStreamSynchronize(S.stream));
    HIPC(hipMemcpy(out, S.res2_cuload, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    // the rim-wave schedule keeps a CU's record as one word behind these (evp_resident2.hip, EVP_RES2_LOCK_CAS): where that word
    // is the last launch's, the record is read out of it, in the same layout
    std::vector<unsigned long long> words(2048);
    HIPC(hipMemcpy(words.data(), S.res2_cuload + 2048 * 8, words.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int cu = 0; cu < 2048 && 8 * cu + 8 <= n; ++cu) {
        const unsigned long long w = words[(size_t)cu];
        if ((unsigned)(w >> 40) != S.res2_epoch) continue;
        int32_t *o = out + 8 * cu;
        o[0] = 0; o[1] = (int32_t)(S.res2_epoch << 12);
        for (int q = 0; q < 4; ++q) o[2 + q] = (int32_t)((w >> (8 * q)) & 255u);
        o[6] = (int32_t)((w >> 32) & 255u); o[7] = 0;
    }
    return 0;
}

// Phase stamps of the last resident launch made with CICE_EVP_HIP_RES_PROF=1: [tiles][4 chunks][8] x u64.
int cice_evp_hip_debug_prof(uint64_t *out, int32_t ntiles_max)
{
    if (!S.ready || !S.res2_prof) return fail(-1, "no profiled resident launch (CICE_EVP_HIP_RES_PROF=1, 16 x 16 tiles)");
    if (!out || ntiles_max < S.res2_ntiles) return fail(-1, "bad argument: need room for %d tiles", S.res2_ntiles);
    HIPC(hipStreamSynchronize(S.stream));
    HIPC(hipMemcpy(out, S.res2_prof, (size_t)S.res2_ntiles * 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return S.res2_ntiles > 0 ? 0 : -1;
}

// Launch stamps of the same launch: [tiles][4 waves][8] x u64 -- 100 MHz wall clock at workgroup start, after the per-CU lock, the
// lane tables and masks, the state loads, the first ring poll, the loop's end, the write-back's end; [7] = chunk | active chunks << 8.
int cice_evp_hip_debug_prof_launch(uint64_t *out, int32_t ntiles_max)
{
    if (!S.ready || !S.res2_prof) return fail(-1, "no profiled resident launch (CICE_EVP_HIP_RES_PROF=1, 16 x 16 tiles)");
    if (!out || ntiles_max < S.res2_ntiles) return fail(-1, "bad argument: need room for %d tiles", S.res2_ntiles);
    HIPC(hipStreamSynchronize(S.stream));
    HIPC(hipMemcpy(out, S.res2_prof + (size_t)S.res2_ntiles * 32, (size_t)S.res2_ntiles * 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return S.res2_ntiles > 0 ? 0 : -1;
}

// Host-only: the lane tables of the resident kernel's rim-wave schedule (rim_plan.h) for ONE block of ni x nj cells with one
// ghost cell all round, closed or cyclic; mask: (ni + 2) x (nj + 2) bytes, bit 0 ice T-cell, bit 1 ice U-cell.  Returns the number
// of tiles (out pointers may be NULL to ask for it), or < 0.  Per tile: perm[256], uperm[256] (255: none), info8 = {|L_T|, |L_U|,
// active chunks, active chunks of the ice-first packing, ok, tiles per row, tiles per column, 0}; cls[256] as resident2_setup's.
int cice_evp_hip_rim_plan(int32_t ni, int32_t nj, int32_t cyclic_ew, int32_t cyclic_ns, const uint8_t *mask, int32_t ntiles_max,
                          uint8_t *perm, uint8_t *uperm, int32_t *info8, uint8_t *cls)
{
    if (ni < 1 || nj < 1 || !mask) return fail(-1, "rim_plan: bad argument");
    rim_plan::Block B;
    rim_plan::block(ni, nj, cyclic_ew != 0, cyclic_ns != 0, mask, B);
    const int nt = B.gx * B.gy;
    if (!perm && !uperm && !info8 && !cls) return nt;
    if (ntiles_max < nt) return fail(-1, "rim_plan: room for %d tiles, %d needed", (int)ntiles_max, nt);
    for (int t = 0; t < nt; ++t) {
        const rim_plan::Tile &tl = B.tiles[(size_t)t];
        if (perm) std::copy(tl.perm, tl.perm + 256, perm + (size_t)t * 256);
        if (uperm) std::copy(tl.uperm, tl.uperm + 256, uperm + (size_t)t * 256);
        if (cls) std::copy(&B.cls[(size_t)t * 256], &B.cls[(size_t)t * 256] + 256, cls + (size_t)t * 256);
        if (info8) {
            const int32_t v[8] = {tl.n_lt, tl.n_lu, tl.nact, tl.nact_packed, tl.ok ? 1 : 0, B.gx, B.gy, 0};
            std::copy(v, v + 8, info8 + (size_t)t * 8);
        }
    }
    return nt;
}

// Host-only: res2_choose (evp_device.h) over n cases that share cap, logw and hooks; bits as in include/cice_evp_hip_testing.h
int cice_evp_hip_debug_res2_choose(int64_t n, const uint32_t *facts, int32_t cap, int32_t logw, int32_t hooks, uint32_t *chosen)
{
    if (n < 0 || !facts || !chosen) return fail(-1, "res2_choose: bad argument");
    for (int64_t e = 0; e < n; ++e) {
        auto bit = [&](int k) { return (facts[e] >> k & 1u) != 0; };
        const unsigned fl = (bit(9) ? EVP_F_WATER_IS_OCN : 0u) | (bit(10) ? EVP_F_TBU_ZERO : 0u);
        const Res2Facts f{bit(0), cap, logw, bit(1), bit(2) ? 1 : 2, bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), fl, bit(11), bit(12), bit(13), bit(14), bit(15), bit(16), bit(17), hooks};
        const Res2Choice c = res2_choose(f);
        chosen[e] = (unsigned)c.v.strict | c.v.remote << 1 | c.v.coop << 2 | c.v.lean << 3 | c.v.rimu << 4 | c.rim_tables << 5 | (unsigned)c.v.logw << 8 | (unsigned)(c.v.cap + 1) << 16;
    }
    return 0;
}

// Host-only: cg_choose_schedule (cgrid_schedule.h) over n rows of facts, see the testing header
int cice_evp_hip_debug_cgrid_choose(int64_t n, const int32_t *facts, int32_t *out)
{
    if (n < 0 || !facts || !out) return fail(-1, "cgrid_choose: bad argument");
    static_assert(sizeof(int) == sizeof(int32_t), "a row of facts is the struct");
    for (int64_t e = 0; e < n; ++e) {
        CgSchedFacts f;
        std::memcpy(&f, facts + e * CG_NFACTS, sizeof f);
        const CgSchedule s = cg_choose_schedule(f);
        std::memcpy(out + e * CG_NSCHED, &s, sizeof s);
    }
    return 0;
}

// Host-only: 1 where the table of evp_resident2.hip has the instantiation
int cice_evp_hip_debug_res2_built(int32_t strict, int32_t cap, int32_t logw, int32_t remote, int32_t coop, int32_t lean, int32_t rimu)
{
    return evp_resident2_kernel({strict != 0, cap, logw, remote != 0, coop != 0, lean != 0, rimu != 0}) != nullptr;
}

// Host-only: build the halo plan for `dims` without touching a device (tests).
int cice_evp_hip_plan_build(const cice_evp_hip_dims *dims)
{
    if (!dims) return fail(-1, "null dims");
    if (!build_halo_plan(*dims, S.plan)) return fail(-3, "halo plan: %s", S.plan.error.c_str());
    build_stress_tfold_xplan(*dims, S.plan, S.stress_x);
    return 0;
}

// tripoleT stress symmetrisation of the plan built last on any rank layout (fold_prep_plan.h), see the testing header
int cice_evp_hip_stress_tfold_xplan(int32_t *info4, int32_t *dst, int32_t *src, int32_t *own_dst, int32_t *own_src,
                                    int32_t *corner_dst, int32_t *corner_src)
{
    const StressTfoldXPlan &X = S.stress_x;
    if (info4) {
        info4[0] = (int32_t)X.dst.size(); info4[1] = (int32_t)X.own_dst.size(); info4[2] = (int32_t)X.corner_dst.size();
        info4[3] = X.collective ? 1 : 0;
    }
    if (!X.ok()) {                                            // declined: the reason is the last error's text
        g_err = X.why;
        return 1;
    }
    copy_out(dst, X.dst); copy_out(src, X.src);
    copy_out(own_dst, X.own_dst); copy_out(own_src, X.own_src);
    copy_out(corner_dst, X.corner_dst); copy_out(corner_src, X.corner_src);
    return 0;
}

// the whole plan built last (PlanDump above; tests/test_halo_plan_digest_cpu.py)
int cice_evp_hip_plan_dump(int32_t *out, int32_t n)
{
    PlanDump count{nullptr};
    count.put(S.plan);
    if (!out) return count.n;
    if (n < count.n) return fail(-1, "plan_dump: room for %d values, %d needed", (int)n, (int)count.n);
    PlanDump dump{out};
    dump.put(S.plan);
    return dump.n;
}

int cice_evp_hip_halo_plan(int32_t *counts4, int32_t *local_dst, int32_t *local_src,
                           int32_t *local_sign, int32_t *peer_rank, int32_t *peer_nsend,
                           int32_t *peer_nrecv, int32_t *send_src, int32_t *recv_dst)
{
    const HaloPlan &P = S.plan;
    copy_out(local_dst, P.local_dst);
    copy_out(local_src, P.local_src);
    copy_out(local_sign, P.local_sign);
    const size_t ns = copy_out(send_src, P.peers, &HaloPeer::send_src), nr = copy_out(recv_dst, P.peers, &HaloPeer::recv_dst);
    for (size_t q = 0; q < P.peers.size(); ++q) {
        if (peer_rank) peer_rank[q] = P.peers[q].rank;
        if (peer_nsend) peer_nsend[q] = (int32_t)P.peers[q].send_src.size();
        if (peer_nrecv) peer_nrecv[q] = (int32_t)P.peers[q].recv_dst.size();
    }
    if (counts4) {
        counts4[0] = (int32_t)P.local_dst.size();
        counts4[1] = (int32_t)P.peers.size();
        counts4[2] = (int32_t)ns;
        counts4[3] = (int32_t)nr;
    }
    return 0;
}

// Tripole part of the plan built by the last init / plan_build (tests): counts3 =
// {pairs, poles, late copies}; lists may be NULL.
int cice_evp_hip_peer_plan(int32_t *send_dst, int32_t *recv_gid)
{
    copy_out(send_dst, S.plan.peers, &HaloPeer::send_dst);
    copy_out(recv_gid, S.plan.peers, &HaloPeer::recv_gid);
    return 0;
}

// The lists the on-chip kernel uses when the tripole fold row is split over ranks (halo_plan.h): per peer (ascending rank,
// as cice_evp_hip_halo_plan) counts4 = {ghost entries at the head of the send list, of the recv list, seam images out, in};
// send_sign in send-list order; the seam images out as (src, dst at the peer, sign), in as (dst, global column, sign).
int cice_evp_hip_fold_images_plan(int32_t *counts4, int32_t *send_sign, int32_t *out3, int32_t *in3)
{
    const std::vector<HaloPeer> &peers = S.plan.peers;
    for (size_t q = 0; counts4 && q < peers.size(); ++q) {
        const HaloPeer &p = peers[q];
        counts4[4 * q] = p.n_ghost_send; counts4[4 * q + 1] = p.n_ghost_recv;
        counts4[4 * q + 2] = (int32_t)p.fimg_src.size(); counts4[4 * q + 3] = (int32_t)p.fimg_recv_dst.size();
    }
    copy_out(send_sign, peers, &HaloPeer::send_sign);
    copy_out(out3, peers, &HaloPeer::fimg_src, 3);
    copy_out(at(out3, 1), peers, &HaloPeer::fimg_dst, 3);
    copy_out(at(out3, 2), peers, &HaloPeer::fimg_sign, 3);
    copy_out(in3, peers, &HaloPeer::fimg_recv_dst, 3);
    copy_out(at(in3, 1), peers, &HaloPeer::fimg_recv_col, 3);
    copy_out(at(in3, 2), peers, &HaloPeer::fimg_recv_sign, 3);
    return 0;
}

// recv_sign of cice_evp_hip_halo_plan's recv list (-1: the ghost lies across the tripole fold), same order
int cice_evp_hip_peer_signs(int32_t *recv_sign)
{
    copy_out(recv_sign, S.plan.peers, &HaloPeer::recv_sign);
    return 0;
}

int cice_evp_hip_center_plan(int32_t *count, int32_t *dst, int32_t *src, int32_t *vsign)
{
    const HaloPlan &P = S.plan;
    const size_t n = copy_out(dst, P.center_dst);
    copy_out(src, P.center_src);
    copy_out(vsign, P.center_vsign);
    if (count) *count = (int32_t)n;
    return P.center_remote ? 1 : 0;
}

// Lists of the shifted-copy exchange (halo_plan.h): which 0 = this rank's cells of row NY-1 where the copy is built,
// 1 = centre-field ghost cells filled from it, 2 = ghost-row cells of the stress symmetrisation filled from it; 3 / 4 =
// east-west ghost cells of row NY and the staging slots that hold their values after a plain exchange.
// Returns 1 when the blocks holding row NY have more than one owner (the exchanges are collective then), else 0.
int cice_evp_hip_fold_split_plan(int32_t which, int32_t *count, int32_t *cells)
{
    const HaloPlan &P = S.plan;
    // (5 / 6: tripoleT -- east-west ghost cells of the top row that the stress symmetrisation leaves as images of their own array,
    // and the cells they mirror; 7 / 8: the north-west corner ghost cells and theirs)
    const std::vector<int32_t> *lists[9] = {&P.fold_shift_cells, &P.center_foldr_dst, &P.stress_foldr_dst, &P.center_seam_dst, &P.center_seam_slot,
                                            &P.stress_own_dst, &P.stress_own_src, &P.stress_corner_dst, &P.stress_corner_src};
    const size_t n = copy_out(cells, *lists[which >= 0 && which < 8 ? which : 8]);
    if (count) *count = (int32_t)n;
    return P.fold_split ? 1 : 0;
}

// The range-proved square root and division of the lean resident loops (evp_range_math.h) beside the compiler's, on the current
// device; needs no cice_evp_hip_init.  Host arrays of n elements.
int cice_evp_hip_debug_range_math(int64_t n, const double *x, const double *num, const double *den, double *sqrt_lib, double *sqrt_core,
                                  double *div_lib, double *div_core, uint8_t *verdict)
{
    if (n < 1 || n > ((int64_t)1 << 26) || !x || !num || !den || !sqrt_lib || !sqrt_core || !div_lib || !div_core || !verdict)
        return fail(-1, "debug_range_math: bad argument");
    const size_t nb = (size_t)n * sizeof(double);
    double *d = nullptr;
    unsigned char *dv = nullptr;
    HIPC(hipMalloc((void **)&d, 7 * nb));
    hipError_t e = hipMalloc((void **)&dv, (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(d, x, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, num, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, den, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = evp_range_math_probe((long long)n, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n, d + 6 * n, dv, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    double *outs[4] = {sqrt_lib, sqrt_core, div_lib, div_core};
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpy(outs[k], d + (3 + k) * n, nb, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(verdict, dv, (size_t)n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (dv) (void)hipFree(dv);
    if (e != hipSuccess) return fail(-2, "debug_range_math: %s", hipGetErrorString(e));
    return 0;
}

int cice_evp_hip_stress_plan(int32_t *count, int32_t *dst, int32_t *src)
{
    const size_t n = copy_out(dst, S.plan.stress_dst);
    copy_out(src, S.plan.stress_src);
    if (count) *count = (int32_t)n;
    return 0;
}
#endif  // CICE_EVP_HIP_TESTING

// General form of the seam step (any rank layout): counts2 = {entries, staging slots}; lists may be NULL.
int cice_evp_hip_seam_fin_plan(int32_t *counts2, int32_t *dst, int32_t *a, int32_t *b, int32_t *coef)
{
    const HaloPlan &P = S.plan;
    if (counts2) { counts2[0] = (int32_t)P.fin_dst.size(); counts2[1] = (int32_t)P.tail; }
    copy_out(dst, P.fin_dst);
    copy_out(a, P.fin_a);
    copy_out(b, P.fin_b);
    copy_out(coef, P.fin_coef);
    return P.stress_remote ? 1 : 0;
}

int cice_evp_hip_march_info(int32_t *out, int32_t n)
{
    const State::March &M = S.march;
    const int32_t v[12] = {M.mode, (int32_t)std::min<long>(M.passes, 0x7fffffffL), M.declined, M.L.nblk ? M.L.plan.me.nstrips : 0, M.L.nseg, M.L.seglen,
                           M.last_call ? 1 : 0, M.direct, M.L.kpass, (int32_t)std::min<long>(M.subcycles, 0x7fffffffL),
                           M.mode == 1 ? M.L.band_rows : 0, M.last_call ? M.call_band_subcycles : 0};
    for (int k = 0; out && k < n && k < 12; ++k) out[k] = v[k];
    return 0;
}

// One line on what the last cice_evp_hip_subcycle ran and why the alternatives did not -- for logs (the Fortran shim
// prints it once after the first call when CICE_EVP_HIP_VERBOSE is set) and for reading a first multi-GPU run.
int cice_evp_hip_describe_path(char *buf, int32_t n)
{
    if (!buf || n < 2) return fail(-1, "describe_path: no buffer");
    const State::March &M = S.march;
    const char *kernel = S.res_mode == 1 ? (S.res_remote ? "on-chip resident (tagged records, neighbours on other ranks)"
                                                       : S.res2_rimu ? "on-chip resident (tagged records; edge U-cells in the rim wave)"
                                                                     : "on-chip resident (tagged records)")
                         : (M.last_call ? (M.L.kpass == 4 ? "four subcycles per pass (marching)" : M.L.kpass == 3 ? "three subcycles per pass (marching)" : "two subcycles per pass (marching)")
                                      : "one subcycle per launch (streaming)");
    const char *transport = S.plan.peers.empty() ? "none (one rank)" : (S.direct.on ? "mailbox over HIP IPC" : (S.have_comm ? "RCCL send/recv" : "not set up"));
    const char *ring = (M.mode == 1 && !S.plan.peers.empty())
                           ? (M.direct == 1 ? " (ring between ranks: stores into HIP-IPC-mapped inboxes)"
                                            : (M.direct == 2 ? " (ring between ranks: RCCL send/recv, direct stores on trial)" : " (ring between ranks: RCCL send/recv)"))
                           : "";
    char band[400] = "";
    if (M.mode == 1 && M.L.fold.H > 0 && S.d.nranks > 1) {
        const char *ovl = env("CICE_EVP_HIP_MARCH_OVERLAP");
        std::snprintf(band, sizeof band, " (tripole: rows 1 .. %d marched, fold band of %d rows one subcycle per launch on %d of %d ranks, %s; its "
                      "velocity halo in lockstep on every rank with the full lists%s)", M.L.fold.zone, M.L.fold.H, M.L.band_ranks, (int)S.d.nranks,
                      M.L.band_rows > 0 ? "this one among them" : "none of it here",
                      (ovl && env_on(ovl, false)) ? "; the overlapped ring is not taken beside a band: serial form" : "");
    } else if (M.mode == 1 && M.L.fold.H > 0)
        std::snprintf(band, sizeof band, " (tripole: rows 1 .. %d marched, fold band of %d rows one subcycle per launch)", M.L.fold.zone, M.L.fold.H);
    std::snprintf(buf, (size_t)n, "rank %d of %d: kernel = %s; halo transport = %s%s%s; marching path: %s%s%s%s%s; blocks %d, cells per exchange %d",
                  (int)S.d.rank, (int)std::max(1, (int)S.d.nranks), kernel, transport,
                  (!S.plan.peers.empty() && !S.direct.on && !S.direct.why.empty()) ? " (mailbox off: " : "",
                  (!S.plan.peers.empty() && !S.direct.on && !S.direct.why.empty()) ? (S.direct.why + ")").c_str() : "",
                  M.mode == 1 ? "on" : (M.mode == 0 ? "off" : "undecided"), (M.mode == 0 && !M.why.empty()) ? " -- " : "",
                  (M.mode == 0 && !M.why.empty()) ? M.why.c_str() : "", ring, band, (int)S.d.nblocks, (int)(S.msk.on ? S.msk.n_send : S.n_send));
    const std::string cg = cgrid_schedule();
    if (!cg.empty()) {
        const size_t used = std::strlen(buf);
        std::snprintf(buf + used, (size_t)n - used, "; %s", cg.c_str());
    }
    return 0;
}

#ifdef CICE_EVP_HIP_TESTING
int cice_evp_hip_plan_flags(int32_t *flags, int32_t n)
{
    const HaloPlan &P = S.plan;
    const int32_t v[5] = {P.any_fold_exchange, P.fold_rows, P.stress_remote, P.center_remote, P.center_fold_remote};
    int32_t k = 0;
    for (; flags && k < n && k < 5; ++k) flags[k] = v[k];
    return k;
}

// The C grid's fold step and exchange lists (halo_plan.h: cg_*), see the testing header
int cice_evp_hip_cgrid_fold_xplan(int32_t loc, int32_t *info4, int32_t *count, int32_t *dst, int32_t *a, int32_t *b, int32_t *flip)
{
    if (loc < 0 || loc > 3) return fail(-1, "bad location %d", (int)loc);
    const HaloPlan &P = S.plan;
    if (info4) {
        info4[0] = P.cg_split ? 1 : 0;
        info4[1] = P.cg_tail;
        info4[2] = (int32_t)P.cg_peers.size();
        info4[3] = 0;
        for (const HaloPeer &p : P.cg_peers) info4[3] += (int32_t)p.send_src.size();
    }
    const FoldList &L = P.cg_fold[loc];
    if (count) *count = (int32_t)L.dst.size();
    copy_out(dst, L.dst);
    copy_out(a, L.a);
    copy_out(b, L.b);
    copy_out(flip, L.flip);
    return 0;
}

int cice_evp_hip_cgrid_fold_xpeers(int32_t *peer5, int32_t *send_src, int32_t *send_dst, int32_t *recv_dst, int32_t *recv_gid)
{
    const std::vector<HaloPeer> &peers = S.plan.cg_peers;
    for (size_t q = 0; peer5 && q < peers.size(); ++q) {
        const HaloPeer &p = peers[q];
        peer5[5 * q] = p.rank; peer5[5 * q + 1] = (int32_t)p.send_src.size(); peer5[5 * q + 2] = (int32_t)p.recv_dst.size();
        peer5[5 * q + 3] = p.n_ghost_send; peer5[5 * q + 4] = p.n_ghost_recv;
    }
    copy_out(send_src, peers, &HaloPeer::send_src);
    copy_out(send_dst, peers, &HaloPeer::send_dst);
    copy_out(recv_dst, peers, &HaloPeer::recv_dst);
    copy_out(recv_gid, peers, &HaloPeer::recv_gid);
    return 0;
}

int cice_evp_hip_seam_plan(int32_t *counts3, int32_t *seam_a, int32_t *seam_b, int32_t *seam_pole,
                           int32_t *late_dst, int32_t *late_src, int32_t *late_sign)
{
    const HaloPlan &P = S.plan;
    if (counts3) {
        counts3[0] = (int32_t)P.seam_a.size();
        counts3[1] = (int32_t)P.seam_pole.size();
        counts3[2] = (int32_t)P.late_dst.size();
    }
    copy_out(seam_a, P.seam_a);
    copy_out(seam_b, P.seam_b);
    copy_out(seam_pole, P.seam_pole);
    copy_out(late_dst, P.late_dst);
    copy_out(late_src, P.late_src);
    copy_out(late_sign, P.late_sign);
    return 0;
}
#endif  // CICE_EVP_HIP_TESTING

}  // extern "C"
