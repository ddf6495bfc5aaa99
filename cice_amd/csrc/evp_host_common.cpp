// Host side, common part: error text, the device state, copies, static metric terms
// (init_dyn_shared), index lists, ghost-image push table, kernel argument block.
#include "evp_host.h"

// host arithmetic of derive_metrics must round every operation (no FMA)
#pragma clang fp contract(off)

// (the kernel objects are compiled once and linked into both libraries: their two switches come through this function)
#ifdef CICE_EVP_HIP_TESTING
const char *evp_env_test(const char *key) { return std::getenv(key); }
#else
const char *evp_env_test(const char *) { return nullptr; }
#endif

namespace evp_host {

std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code ? code : -1;
}

State S;

cice_evp_hip_dims host_dims()
{
    cice_evp_hip_dims d = S.d;
    d.ilo = S.ilo.data(); d.ihi = S.ihi.data(); d.jlo = S.jlo.data(); d.jhi = S.jhi.data();
    d.iglob0 = S.iglob0.data(); d.jglob0 = S.jglob0.data();
    return d;
}

// The device memory (S.mem), then what is not memory.  The caller resets the state itself (S = State()).
void free_all()
{
    S.mem.free_all();
    for (void *q : S.direct.opened) (void)hipIpcCloseMemHandle(q);
    for (auto &kv : S.graphs) (void)hipGraphExecDestroy(kv.second);
    for (hipEvent_t e : {S.ev0, S.ev1, S.ev2, S.ev3, S.evm[0], S.evm[1], S.ev_pack, S.ev_halo})
        if (e) (void)hipEventDestroy(e);
    if (S.have_comm) (void)ncclCommDestroy(S.comm);
    for (auto &kv : S.pinned) (void)hipHostUnregister(const_cast<void *>(kv.first));
    if (S.stream_comm) (void)hipStreamDestroy(S.stream_comm);
    if (S.stream) (void)hipStreamDestroy(S.stream);
}

// Copies blocks 1..nblocks of a host (nx,ny,max_blocks) array: contiguous prefix.
int h2d(double *dst, const double *src)
{
    HIPC(hipMemcpyAsync(dst, src, S.n * sizeof(double), hipMemcpyHostToDevice, S.stream));
    return 0;
}
int d2h(double *dst, const double *src)
{
    HIPC(hipMemcpyAsync(dst, src, S.n * sizeof(double), hipMemcpyDeviceToHost, S.stream));
    return 0;
}

// Device view of a caller's array if it lies inside a range registered (and mapped) by cice_evp_hip_pin_host
static void *mapped_view(const void *host, size_t bytes)
{
    auto it = S.pinned.upper_bound(host);
    if (it == S.pinned.begin()) return nullptr;
    --it;
    const char *base = (const char *)it->first;
    if (!it->second.dev || (const char *)host < base || (const char *)host + bytes > base + it->second.bytes) return nullptr;
    return (char *)it->second.dev + ((const char *)host - base);
}

static int run_batch(CopyBatch &B, bool to_device)
{
    const bool off = !env_on(env_test("CICE_EVP_HIP_GATHER"), true);
    EvpCopyTab T{};
    T.len = S.n;
    T.vec2 = 1;
    auto flush = [&]() {
        if (T.n > 0) evp_launch_copy_many(T, S.stream);
        T.n = 0;
        T.vec2 = 1;
    };
    for (auto &it : B.items) {
        double *dst = it.first;
        const double *src = it.second;
        const void *host = to_device ? (const void *)src : (const void *)dst;
        void *view = off ? nullptr : mapped_view(host, S.n * sizeof(double));
        if (!view) {
            if (to_device ? h2d(dst, src) : d2h(dst, src)) return -1;
            continue;
        }
        T.src[T.n] = to_device ? (const double *)view : src;
        T.dst[T.n] = to_device ? dst : (double *)view;
        if ((((uintptr_t)T.src[T.n]) | ((uintptr_t)T.dst[T.n])) & 15u) T.vec2 = 0;
        if (++T.n == EVP_COPY_MAX) flush();
    }
    flush();
    HIPC(hipGetLastError());
    B.items.clear();
    return 0;
}
// every host array of the batch lies in a range the caller page-locked and mapped (and the gather path is on)
bool batch_mapped(const CopyBatch &B, bool to_device)
{
    if (!env_on(env_test("CICE_EVP_HIP_GATHER"), true)) return false;
    for (auto &it : B.items)
        if (!mapped_view(to_device ? (const void *)it.second : (const void *)it.first, S.n * sizeof(double))) return false;
    return true;
}
// device -> mapped host arrays, only the cells whose mask byte has `bit` set (batch_mapped(B, false) must hold)
int d2h_batch_masked(CopyBatch &B, unsigned bit)
{
    EvpCopyTab T{};
    T.len = S.n;
    for (auto &it : B.items) {
        T.src[T.n] = it.second;
        T.dst[T.n] = (double *)mapped_view(it.first, S.n * sizeof(double));
        if (++T.n == EVP_COPY_MAX) { evp_launch_copy_many_masked(T, S.mask, bit, S.stream); T.n = 0; }
    }
    evp_launch_copy_many_masked(T, S.mask, bit, S.stream);
    HIPC(hipGetLastError());
    B.items.clear();
    return 0;
}
int h2d_batch(CopyBatch &B) { return run_batch(B, true); }
int d2h_batch(CopyBatch &B) { return run_batch(B, false); }

// Static metric terms, host arithmetic in the reference's operation order
// (init_dyn_shared, ice_dyn_shared.F90:384-388, 401-441).  dxhy/dyhx are
// evaluated directly on the N/E ghost T-cells from the HTE/HTN ghost values
// (which CICE defines from the global arrays, ice_grid.F90:662-666) instead of
// through a halo update: same operands, same result for every cell that can
// hold ice.
int derive_metrics(const double *HTE, const double *HTN, const double *dxT, const double *dyT,
                   const double *uarear, const double *tarea)
{
    const int nx = S.d.nx_block;
    const size_t plane = S.plane;
    std::vector<std::vector<double>> m(7, std::vector<double>(S.n, 0.0));   // cxp cyp cxm cym dxhy dyhx Dmin
    const double p5 = 0.5, c1p5 = 1.5;
    for (int b = 0; b < S.d.nblocks; ++b) {
        const double *hte = HTE + b * plane, *htn = HTN + b * plane;
        for (size_t k = 0; k < plane; ++k) m[6][b * plane + k] = S.prm.deltaminEVP * tarea[b * plane + k];
        for (int j = S.jlo[b]; j <= S.jhi[b] + 1; ++j)
            for (int i = S.ilo[b]; i <= S.ihi[b] + 1; ++i) {
                const size_t c = (size_t)(j - 1) * nx + (i - 1);
                const size_t g = b * plane + c;
                m[0][g] = (c1p5 * htn[c] - p5 * htn[c - nx]);        // cxp
                m[1][g] = (c1p5 * hte[c] - p5 * hte[c - 1]);         // cyp
                m[2][g] = -(c1p5 * htn[c - nx] - p5 * htn[c]);       // cxm
                m[3][g] = -(c1p5 * hte[c - 1] - p5 * hte[c]);        // cym
                m[4][g] = p5 * (hte[c] - hte[c - 1]);                // dxhy
                m[5][g] = p5 * (htn[c] - htn[c - nx]);               // dyhx
            }
    }
    if (h2d(S.stat[0], dxT) || h2d(S.stat[1], dyT) || h2d(S.stat[9], uarear)) return -1;
    if (h2d(S.hte, HTE) || h2d(S.htn, HTN)) return -1;
    // in-kernel metric terms need tarea == dxT*dyT bit for bit (ice_grid.F90:681)
    bool same = true;
    for (size_t k = 0; k < S.n && same; ++k) same = (tarea[k] == dxT[k] * dyT[k]);
    if (same) S.flags |= EVP_F_METRICS;
    // on the tripole ghost row dxhy/dyhx are mirrored interior values (halo update with sign,
    // ice_dyn_shared.F90:412-417), not a local difference: keep them as arrays there
    if (S.d.ns_boundary_type == CICE_EVP_BND_TRIPOLE || S.d.ns_boundary_type == CICE_EVP_BND_TRIPOLET) S.flags |= EVP_F_DXHY_ARRAY;
    const int order[7] = {4, 5, 6, 7, 2, 3, 8};   // stat slots of cxp cyp cxm cym dxhy dyhx Dmin
    for (int k = 0; k < 7; ++k)
        if (h2d(S.stat[order[k]], m[k].data())) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

int upload_lists()
{
    const HaloPlan &P = S.plan;
    // a list on the device; an empty one stays a null pointer
    auto up = [&](const auto &v, auto *&dptr) -> int { return v.empty() ? 0 : S.mem.upload(dptr, v); };
    S.n_local = (int)P.local_dst.size();
    if (up(P.local_dst, S.h_local_dst) || up(P.local_src, S.h_local_src) || up(P.local_sign, S.h_local_sign)) return -1;
    S.n_seam = (int)P.seam_a.size();
    S.n_pole = (int)P.seam_pole.size();
    S.n_late = (int)P.late_dst.size();
    if (up(P.seam_a, S.h_seam_a) || up(P.seam_b, S.h_seam_b) || up(P.seam_pole, S.h_seam_pole) ||
        up(P.late_dst, S.h_late_dst) || up(P.late_src, S.h_late_src)) return -1;
    S.n_stress = (int)P.stress_dst.size();
    if (up(P.stress_dst, S.h_stress_dst) || up(P.stress_src, S.h_stress_src)) return -1;
    S.n_stress_own = (int)P.stress_own_dst.size();
    if (up(P.stress_own_dst, S.h_stress_own_dst) || up(P.stress_own_src, S.h_stress_own_src)) return -1;
    S.n_stress_corner = (int)P.stress_corner_dst.size();
    if (up(P.stress_corner_dst, S.h_stress_corner_dst) || up(P.stress_corner_src, S.h_stress_corner_src)) return -1;
    if (up(P.late_sign, S.h_late_sign)) return -1;
    S.n_fin = (int)P.fin_dst.size();
    // the list is only run on layouts that split the seam row (halo_uv: general form) or when forced for tests
    const bool fin_used = P.tail > 0 || env_on(env_test("CICE_EVP_HIP_SEAM_FIN"), false);
    if (fin_used && S.n_fin > evp_halo_seam_fin_capacity()) return fail(-3, "tripole seam: %d cells to finalise on one rank (limit %d)", S.n_fin, evp_halo_seam_fin_capacity());
    if (up(P.fin_dst, S.h_fin_dst) || up(P.fin_a, S.h_fin_a) || up(P.fin_b, S.h_fin_b)) return -1;
    if (up(P.fin_coef, S.h_fin_coef)) return -1;
    std::vector<int32_t> ss, rd;
    std::vector<int8_t> rs;
    for (const HaloPeer &p : P.peers) {
        ss.insert(ss.end(), p.send_src.begin(), p.send_src.end());
        rd.insert(rd.end(), p.recv_dst.begin(), p.recv_dst.end());
        rs.insert(rs.end(), p.recv_sign.begin(), p.recv_sign.end());
    }
    S.n_send = (int)ss.size();
    S.n_recv = (int)rd.size();
    if (up(ss, S.h_send_src) || up(rd, S.h_recv_dst) || up(rs, S.h_recv_sign)) return -1;
    if (S.n_send && S.mem.alloc(S.sendbuf, 2 * ss.size())) return -1;
    if (S.n_recv && S.mem.alloc(S.recvbuf, 2 * rd.size())) return -1;
    if (P.cg_split) {        // the C grid's exchange (HaloPlan::cg_peers)
        std::vector<int32_t> cs, cr;
        std::vector<int8_t> cg;
        for (const HaloPeer &p : P.cg_peers) {
            cs.insert(cs.end(), p.send_src.begin(), p.send_src.end());
            cr.insert(cr.end(), p.recv_dst.begin(), p.recv_dst.end());
            cg.insert(cg.end(), p.recv_sign.begin(), p.recv_sign.end());
        }
        State::CgX &X = S.cgx;
        X.n_send = (int)cs.size();
        X.n_recv = (int)cr.size();
        if (up(cs, X.send_src) || up(cr, X.recv_dst) || up(cg, X.recv_sign)) return -1;
        if (X.n_send && S.mem.alloc(X.sendbuf, 2 * cs.size())) return -1;
        if (X.n_recv && S.mem.alloc(X.recvbuf, 2 * cr.size())) return -1;
    }
    return 0;
}

// Inverse of the local part of the halo plan: for every interior edge cell the
// ghost cells that mirror it, so that the thread producing the cell can store the
// images itself.  Per block 2*(nj+ni) edge slots (W, E, S, N) x 2 entries; an entry is
// dst*2 + (sign<0), or -1.  Falls back to the gather kernel if an image does not fit.
int build_push_table()
{
    const HaloPlan &P = S.plan;
    S.push_ok = false;
    S.push_ni = S.max_ni;
    S.push_nj = S.max_nj;
    const int nslot = 2 * (S.push_nj + S.push_ni);
    std::vector<int> tab((size_t)S.d.nblocks * nslot * 2, -1);
    const int nx = S.d.nx_block;
    bool ok = true;
    for (size_t k = 0; k < P.local_dst.size() && ok; ++k) {
        const int src = P.local_src[k];
        if (src < 0) { ok = false; break; }
        const int b = (int)(src / S.plane);
        const int rem = (int)(src % S.plane);
        const int j = rem / nx + 1, i = rem % nx + 1;
        int cand[4];
        cand[0] = (i == S.ilo[b]) ? (j - S.jlo[b]) : -1;
        cand[1] = (i == S.ihi[b]) ? S.push_nj + (j - S.jlo[b]) : -1;
        cand[2] = (j == S.jlo[b]) ? 2 * S.push_nj + (i - S.ilo[b]) : -1;
        cand[3] = (j == S.jhi[b]) ? 2 * S.push_nj + S.push_ni + (i - S.ilo[b]) : -1;
        const int enc = P.local_dst[k] * 2 + (P.local_sign[k] < 0 ? 1 : 0);
        bool placed = false;
        for (int e = 0; e < 4 && !placed; ++e) {
            if (cand[e] < 0) continue;
            for (int w = 0; w < 2 && !placed; ++w) {
                int &slot = tab[((size_t)b * nslot + cand[e]) * 2 + w];
                if (slot < 0) { slot = enc; placed = true; }
            }
        }
        if (!placed) ok = false;
    }
    if (!ok || P.local_dst.empty()) return 0;
    if (S.mem.upload(S.push, tab)) return -1;
    S.push_ok = true;
    return 0;
}

void fill_args(EvpArgs &A, int cur, int last)
{
    const cice_evp_hip_params &q = S.prm;
    A.p = {q.arlx1i, q.denom1, q.brlx, q.revp, q.e_factor, q.epp2i, q.capping, q.Ktens,
           q.u0, q.cosw, q.sinw, q.rhow};
    A.nx = S.d.nx_block;
    A.ny = S.d.ny_block;
    A.plane = S.plane;
    A.last = last;
    A.tile_list = nullptr;
    A.tile_count = 0;
    A.dx = nullptr; A.dx_count = nullptr; A.dx_fseq = nullptr; A.dx_nb = 0;
    A.blk = S.blk;
    A.mask = S.mask;
    A.u_in = S.u[cur];
    A.v_in = S.v[cur];
    A.u_out = S.u[cur ^ 1];
    A.v_out = S.v[cur ^ 1];
    for (int k = 0; k < 12; ++k) {
        A.sig_in[k] = S.sig[cur][k];
        A.sig_out[k] = S.sig[cur ^ 1][k];
    }
    A.dxT = S.stat[0]; A.dyT = S.stat[1]; A.dxhy = S.stat[2]; A.dyhx = S.stat[3];
    A.cxp = S.stat[4]; A.cyp = S.stat[5]; A.cxm = S.stat[6]; A.cym = S.stat[7];
    A.DminTarea = S.stat[8]; A.uarear = S.stat[9];
    A.HTE = S.hte; A.HTN = S.htn; A.deltaminEVP = q.deltaminEVP;
    A.vrelfac = S.vrelfac;
    A.flags = S.flags & S.flags_allowed;
    if (!S.push_ok) A.flags &= ~EVP_F_PUSH;
    A.push = S.push; A.push_ni = S.push_ni; A.push_nj = S.push_nj;
    A.strength = S.in[F_STRENGTH]; A.Cw = S.in[F_CW]; A.aiX = S.in[F_AIX];
    A.uocn = S.in[F_UOCN]; A.vocn = S.in[F_VOCN]; A.waterx = S.in[F_WATERX];
    A.watery = S.in[F_WATERY]; A.forcex = S.in[F_FORCEX]; A.forcey = S.in[F_FORCEY];
    A.umassdti = S.in[F_UMASSDTI]; A.fm = S.in[F_FM]; A.TbU = S.in[F_TBU];
    A.uvel_init = S.in[F_UVEL_INIT]; A.vvel_init = S.in[F_VVEL_INIT];
    A.strintx = S.in[F_STRINTX]; A.strinty = S.in[F_STRINTY];
    A.taubx = S.in[F_TAUBX]; A.tauby = S.in[F_TAUBY];
}

// Arithmetic variant of the kernels (template MODE, evp_math.h): 3 = capping == 1 and the reference's
// default scalars -- classic EVP (revp == 0), Ktens == 0, cosw == 1, sinw == 0 -- whose products with
// exactly 1.0 / sums with exactly 0.0 the kernels then leave out, bit-neutral (CICE_EVP_HIP_SIMPLE=0: off)
int cap_mode()
{
    const bool simple_ok = env_on(env_test("CICE_EVP_HIP_SIMPLE"), true);
    if (simple_ok && S.prm.capping == 1.0 && S.prm.revp == 0.0 && S.prm.Ktens == 0.0 && S.prm.cosw == 1.0 &&
        S.prm.sinw == 0.0)
        return 3;
    if (S.prm.capping == 1.0) return 1;
    if (S.prm.capping == 0.0) return 0;
    return -1;
}

}  // namespace evp_host
