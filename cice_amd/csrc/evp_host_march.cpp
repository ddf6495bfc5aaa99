// =====================================================================
// Host side of the several-subcycles-per-pass kernel (evp_march.hip): the device-private rectangle layout, the
// conversions between it and the CICE block layout, and the loop.
//
// Strip-major layout: all blocks of the rank are assembled into ONE rectangle of nxr x nyr cells, cut into strips of
// `own` <= 56 columns; per (row, strip) one contiguous block [field][64 lanes] -- with P = EVP_MARCH_PAD = 4, lanes
// P .. P+own-1 are the strip's own columns, the others duplicate its neighbours' (or, beyond a closed side, hold the
// caller's ghost values / zeros).
// Buffers: state (u, v, 12 stresses; two copies), constants of a call (13 fields), optional operands (5), diagnostics
// (4); rows -P .. nyr+P+2 (P halo rows below, P above, two spare rows the prefetch may touch, one dump row).  Every
// cell of the rank exists once: the reference's redundant copies (ghost cells, the T-cells of the north / east fringe
// every block computes for itself, ice_dyn_shared.F90:740-749) are images of it.  The byte mask stays row-major.
//
// A call of cice_evp_hip_subcycle(ndte) through this path:
//   [ndte = Kq + 1: one subcycle with the one-subcycle kernel]  gather -> consistency check (first call after an upload)
//   -> q passes of K = 2 .. 4 subcycles and one of the remaining 2 .. K - 1 (ping-pong between two sets of u, v, 12
//   stresses) -> scatter.  What is decided from the dims alone -- the rectangle, the rim, K, the segments, the lists and the
//   order of passes and exchanges -- comes from march_plan.cpp (build_march_layout, march_schedule); this file is the plumbing.
// Not eligible (the one-subcycle kernels keep running): cyclic north-south boundary, blocks
// that do not tile a rectangle per rank (eliminated land blocks), metric terms (dxhy, dyhx) handed over as arrays that are not
// what the kernel derives from HTE / HTN on the rows it evaluates, a rank too thin next to a closed boundary for its redundant
// rim (march_plan.cpp), a caller whose ghost values are not images of one global state.  Several ranks: the ring of ext + P
// cells travels over RCCL send / recv once per ext + P subcycles (section 6).
//
// Tripole / tripoleT grid on one rank (march_plan.h: MarchFold): the fold does not go into the marching kernel.  The rectangle is
// the ZONE, global rows 1 .. NY - H, closed in the south and with a "neighbour" in the north that is this process's own fold BAND:
// the top H rows and the ghost row beyond the fold stay in the caller's block layout and advance one subcycle at a time with what
// runs tripole grids anyway -- the tile kernel over a tile list that covers the band and ext + P rows below it, then halo_uv (seam
// averaging, mirrored ghost row, images between blocks, the cyclic wrap).  Serial on one stream: a pass of K subcycles, then K band
// subcycles.  Every ext + P subcycles the ring between the two travels on the device (march_scatter / march_gather over row
// windows): the zone's rows under the band into the block layout, the band's rows above the zone into the rectangle; in between
// each side loses one row of validity per subcycle and never reads a lost row for a cell it owns.  The call ends with the
// scatter of the zone's rows into the ping-pong buffer the band's last subcycle wrote.
//
// The same grid on SEVERAL ranks (march_plan.h: build_march_plan, ranks_fold): one zone and one band for the grid, the band on the
// ranks whose blocks reach above the zone, each over its own columns.  A band subcycle is the tile kernel over the band's tiles and
// halo_uv in its remote form, which EVERY rank runs in lockstep with the lists of the one-subcycle loop -- a rank without band rows
// only exchanges, and flips its ping-pong buffer with the others.  At a trade: band rows into the rectangle (gather), then the rank
// ring -- which also carries the corner cells above the zone, out of the rows just gathered on the rank that owns them -- then zone
// rows into the block layout (scatter), whose ghost columns and east-fringe stresses at a rank's x-edges come from the ring cells the
// exchange has just brought.  Runs when asked for (CICE_EVP_HIP_MARCH=1); the overlapped ring is not taken beside a band.
// =====================================================================
#include "evp_host.h"

static_assert(MARCH_PLAN_PAD == EVP_MARCH_PAD && MARCH_PLAN_OWN == EVP_MARCH_OWN && MARCH_PLAN_S_NF == EVP_MARCH_S_NF &&
                  MARCH_PLAN_NODUP == EVP_MARCH_NODUP && MARCH_PLAN_MAXPEER == EVP_MARCH_DIRECT_MAXPEER,
              "march_plan.h and evp_device.h must agree on the strip-major layout");
static_assert(sizeof(MarchOrg) == sizeof(int2) && sizeof(MarchItem) == sizeof(int4), "the layout's tables are uploaded as they are");

namespace evp_host {

namespace {

struct MarchBuf {
    DevicePool mem;              // every device allocation behind a pointer of this struct
    double *st[2] = {};          // state blocks: u v sig x 12
    double *cst = nullptr;       // dxT dyT strength HTE HTN vrelfac uocn vocn forcex forcey umassdti fm uarear
    double *opt = nullptr;       // waterx watery TbU uvel_init vvel_init
    double *diag = nullptr;      // strintx strinty taubx tauby
    uint8_t *mask = nullptr;     // row-major
    unsigned *bad = nullptr, *dup = nullptr;
    int *blkid = nullptr;
    int2 *org = nullptr;
    // the two-cell ring between ranks
    int *send_pos = nullptr, *recv_pos1 = nullptr, *recv_pos2 = nullptr, *send_midx = nullptr, *recv_midx = nullptr;
    double *sendbuf = nullptr, *recvbuf = nullptr;
    // the early launch of an exchange pass: work items that cover every cell other ranks receive from this one
    int4 *band_items = nullptr, *rest_items = nullptr;      // ... and every other (strip, row) of the rectangle
    std::map<int, std::pair<int *, int>> fold_tiles;        // fold band: tile list of the one-subcycle kernel, by tile variant
    hipEvent_t ev_in = nullptr, ev_main = nullptr, ev_done = nullptr;
    // the same ring as stores into the peers' HIP-IPC-mapped inboxes (march_direct_setup)
    void *dx_area = nullptr;     // fine-grained: flag lines | count | err | inbox [2][n_recv * NF]
    std::vector<void *> dx_mapped;
    EvpMarchDirect dx{};
    unsigned dx_seq = 0;
    EvpRingCuts cut_send{}, cut_recv{};      // where each neighbour's block begins in the send / receive list
};
MarchLayout &L = S.march.L;      // the one layout: march_geometry builds it, march_free resets it with the rest of S.march
// slots of the constants block (evp_march.hip: C_*), of the optional block (O_*)
enum { C_DXT = 0, C_DYT, C_STRENGTH, C_HTE, C_HTN, C_VRELFAC, C_UOCN, C_VOCN, C_FORCEX, C_FORCEY, C_UMASSDTI, C_FM, C_UAREAR };
enum { O_WATERX = 0, O_WATERY, O_TBU, O_UINIT, O_VINIT };
MarchBuf B;

// the direct ring's mappings and inbox (a change of the switch re-opens the set-up)
void direct_close()
{
    for (void *m : B.dx_mapped) (void)hipIpcCloseMemHandle(m);
    B.dx_mapped.clear();
    B.mem.free_one(B.dx_area);
    B.dx = EvpMarchDirect{};
    B.dx_seq = 0;
}

}  // namespace

void march_free()
{
    direct_close();
    B.mem.free_all();
    for (hipEvent_t e : {B.ev_in, B.ev_main, B.ev_done})
        if (e) (void)hipEventDestroy(e);
    B = MarchBuf();
    S.march = State::March{};
}

size_t march_allocs() { return B.mem.owned.size(); }

// ---- switches --------------------------------------------------------------------------------------------------------
// CICE_EVP_HIP_MARCH: 0 never, 1 whenever the layout allows, not set (-1): where it pays (march_wanted)
static int march_asked() { return env_int(env("CICE_EVP_HIP_MARCH"), -1); }
// the early launch of an exchange pass (march_run); read on each rank for itself: every rank must be given the same value
static bool march_overlap_asked() { return env_on(env("CICE_EVP_HIP_MARCH_OVERLAP"), false); }
// CICE_EVP_HIP_VERBOSE (set at all): one line on stderr
static void verbose(const char *fmt, ...)
{
    if (!env("CICE_EVP_HIP_VERBOSE")) return;
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "[cice_evp_hip] %s\n", buf);
}
// (test build) the ring between ranks as stores into HIP-IPC-mapped inboxes
static bool march_direct_asked() { return env_on(env_test("CICE_EVP_HIP_MARCH_DIRECT"), false); }
// (test build) what the layout may be asked for: own_max, wrap_inside, ext, kpass, seglen, bandseg; and the tile height in use
static MarchAsk march_ask()
{
    return MarchAsk{env_int(env_test("CICE_EVP_HIP_MARCH_OWN"), EVP_MARCH_OWN), !env_on(env_test("CICE_EVP_HIP_MARCH_SELFX"), false),
                    env_int(env_test("CICE_EVP_HIP_MARCH_EXT"), MARCH_ASK_UNSET), env_int(env_test("CICE_EVP_HIP_MARCH_K"), MARCH_ASK_UNSET),
                    env_int(env_test("CICE_EVP_HIP_MARCH_SEG"), 0), env_int(env_test("CICE_EVP_HIP_MARCH_BANDSEG"), 0), S.tyb % 100};
}

// Are the metric terms the one-subcycle kernels read from arrays (cxp, cyp, cxm, cym, dxhy, dyhx, deltaminEVP * tarea) what the
// marching kernel derives from HTE, HTN, dxT, dyT (evp_cell.inc: metrics) on every T-cell of the global rows below `nrows`?  On a
// tripole grid dxhy / dyhx carry mirrored values on the ghost row beyond the fold (evp_host_common.cpp: derive_metrics,
// cice_evp_hip_set_metrics), and on a tripoleT grid tarea is not dxT * dyT on the top physical row -- rows the zone never
// evaluates.  Once, on the host; the flags EVP_F_METRICS / EVP_F_DXHY_ARRAY speak for the whole domain and are not asked.
static bool metrics_hold(int nrows)
{
    const size_t bytes = S.n * sizeof(double);
    auto down = [&](const double *dev, std::vector<double> &h) -> bool {
        h.resize(S.n);
        if (hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    };
    std::vector<double> hte, htn, dxT, dyT, arr;
    if (!down(S.hte, hte) || !down(S.htn, htn) || !down(S.stat[0], dxT) || !down(S.stat[1], dyT)) return false;
    const int nx = S.d.nx_block;
    const double p5 = 0.5, c1p5 = 1.5, dmin = S.prm.deltaminEVP;
    for (int k = 2; k <= 8; ++k) {           // stat slots: dxhy dyhx cxp cyp cxm cym DminTarea
        if (!down(S.stat[k], arr)) return false;
        for (int b = 0; b < S.d.nblocks; ++b)
            for (int j = S.jlo[b]; j <= S.jhi[b] + 1; ++j) {
                if (S.jglob0[b] - 1 + (j - S.jlo[b]) >= nrows) break;
                for (int i = S.ilo[b]; i <= S.ihi[b] + 1; ++i) {
                    const size_t c = (size_t)b * S.plane + (size_t)(j - 1) * nx + (i - 1);
                    double e;
                    switch (k) {
                    case 2: e = p5 * (hte[c] - hte[c - 1]); break;
                    case 3: e = p5 * (htn[c] - htn[c - nx]); break;
                    case 4: e = (c1p5 * htn[c] - p5 * htn[c - nx]); break;
                    case 5: e = (c1p5 * hte[c] - p5 * hte[c - 1]); break;
                    case 6: e = -(c1p5 * htn[c - nx] - p5 * htn[c]); break;
                    case 7: e = -(c1p5 * hte[c - 1] - p5 * hte[c]); break;
                    default: { const double tarea = dxT[c] * dyT[c]; e = dmin * tarea; }
                    }
                    if (std::memcmp(&e, &arr[c], 8) != 0) return false;
                }
            }
    }
    return true;
}

// Can this rank's sub-domain be held as one rectangle?  Builds the layout and fills S.march.G (host fields) when it can.
static bool march_geometry(std::string &why)
{
    const cice_evp_hip_dims &d = S.d;
    if (!build_march_layout(d, march_ask(), L)) { why = L.why; return false; }
    // ... and what only this process knows; a layout refused here leaves no more behind than the pass size it had settled on
    auto refuse = [&](const char *w) {
        MarchLayout none;
        none.kpass = L.kpass;
        L = none;
        why = w;
        return false;
    };
    if (!L.plan.peers.empty() && !S.have_comm && !S.test_xchg) return refuse("cells of other ranks needed but no RCCL communicator (cice_evp_hip_comm_init)");
    // The kernel derives every metric term from HTE, HTN, dxT, dyT.  A closed grid: tarea == dxT * dyT was verified on every cell
    // at init (EVP_F_METRICS) and nothing else stands in the arrays.  A tripole grid: the arrays differ from that on the ghost row
    // beyond the fold (and, tripoleT, on the top physical row), so the test is the thing itself -- the terms hold on every row
    // the zone evaluates: its own, the redundant rim and the ring.
    if (L.fold.H > 0) {
        if (!metrics_hold(L.fold.to_rect[1])) return refuse("the metric arrays are not what HTE, HTN, dxT, dyT give on the rows the marching kernel evaluates");
    } else if (!(S.flags & EVP_F_METRICS) || (S.flags & EVP_F_DXHY_ARRAY)) return refuse("metric terms come from arrays");
    if (d.nblocks < 1) return refuse("no blocks");
    EvpMarchGeo &G = S.march.G;
    const MarchPlan &P = L.plan;
    G.nxr = P.me.nxr; G.nyr = P.me.nyr; G.ldx = L.ldx; G.rows = L.rows; G.own = P.me.own; G.nstrips = P.me.nstrips;     // held: own cells + rim
    G.nxb = d.nx_block; G.nyb = d.ny_block; G.plane = (int)S.plane; G.nblocks = d.nblocks;
    G.bsx = L.bsx; G.bsy = L.bsy; G.nbx = L.nbx; G.nby = L.nby;
    G.ilo = d.nghost + 1;
    G.wrapx = P.wrapx ? 1 : 0;
    G.gx0 = P.me.gx0; G.gy0 = P.me.gy0; G.nxg = d.nx_global; G.nyg = d.ny_global;
    G.ew_cyclic = d.ew_boundary_type == CICE_EVP_BND_CYCLIC ? 1 : 0;
    G.ext_w = P.ext_w; G.ext_s = P.ext_s; G.nxo = P.owned.nxr; G.nyo = P.owned.nyr;
    G.nyblk = P.owned.nyr + L.band_rows;   // (a fold band on this rank: the blocks go on above the zone, and the ring above it is read from them)
    return true;
}

// The buffers by the layout's sizes, its tables and lists as they are.
static int march_alloc()
{
    State::March &M = S.march;
    auto A = [&](double *&p, int nf) -> int {
        if (p) return 0;
        return B.mem.alloc(p, L.nblk * (size_t)nf * 64, true);
    };
    if (A(B.st[0], EVP_MARCH_S_NF) || A(B.st[1], EVP_MARCH_S_NF) || A(B.cst, EVP_MARCH_C_NF) || A(B.opt, EVP_MARCH_O_NF) ||
        A(B.diag, EVP_MARCH_D_NF)) return -1;
    if (!B.mask && B.mem.alloc(B.mask, (size_t)M.G.rows * M.G.ldx, true)) return -1;
    if (!B.bad && B.mem.alloc(B.bad, 1)) return -1;
    if (!B.blkid && (B.mem.upload(B.blkid, L.blkid) || B.mem.upload(B.org, L.org) || B.mem.upload(B.dup, L.dup))) return -1;
    if (L.plan.n_send + L.plan.n_recv > 0 && !B.sendbuf) {
        if (B.mem.upload(B.send_pos, L.send_pos) || B.mem.upload(B.recv_pos1, L.recv_pos1) || B.mem.upload(B.recv_pos2, L.recv_pos2) ||
            B.mem.upload(B.send_midx, L.send_midx) || B.mem.upload(B.recv_midx, L.recv_midx)) return -1;
        B.cut_send.n = B.cut_recv.n = (int)L.plan.peers.size();
        std::copy(std::begin(L.cut_send), std::end(L.cut_send), B.cut_send.start);
        std::copy(std::begin(L.cut_recv), std::end(L.cut_recv), B.cut_recv.start);
        if (B.mem.alloc(B.sendbuf, std::max<size_t>(L.plan.n_send, 1) * EVP_MARCH_S_NF) ||
            B.mem.alloc(B.recvbuf, std::max<size_t>(L.plan.n_recv, 1) * EVP_MARCH_S_NF)) return -1;
        // the two launches of an overlapped exchange pass (march_run)
        if (!L.band_items.empty() && B.mem.upload(B.band_items, L.band_items)) return -1;
        if (!L.rest_items.empty() && B.mem.upload(B.rest_items, L.rest_items)) return -1;
        for (hipEvent_t *e : {&B.ev_in, &B.ev_main, &B.ev_done})
            if (!*e) HIPC(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    M.G.blkid = B.blkid;
    M.G.blk_org = B.org;
    M.G.blk = S.blk;
    return 0;
}

// One transfer between the ranks of L.plan.peers on stream `st`: to / from each, in the plan's order, nf doubles per cell of its send /
// receive list (per_cell) or nf doubles flat, out of `send` into `recv` (device buffers, the peers' shares one after the other).
// ncclGroupStart{ncclSend, ncclRecv per neighbour}ncclGroupEnd, or (test hook) host buffers and the caller's callback.
static int ring_transfer(const double *send, double *recv, int nf, hipStream_t st, bool per_cell = true)
{
    auto count = [&](size_t cells) { return (per_cell ? cells : (size_t)1) * nf; };
    if (S.test_xchg) {
        std::vector<int32_t> ranks;
        std::vector<int64_t> ns, nr;
        size_t ts = 0, tr = 0;
        for (const MarchPeer &p : L.plan.peers) {
            ranks.push_back(p.rank);
            ns.push_back((int64_t)count(p.send_pos.size()));
            nr.push_back((int64_t)count(p.recv_pos1.size()));
            ts += (size_t)ns.back(); tr += (size_t)nr.back();
        }
        S.test_send.resize(ts + 1);
        S.test_recv.resize(tr + 1);
        HIPC(hipMemcpyAsync(S.test_send.data(), send, ts * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPC(hipStreamSynchronize(st));
        if (S.test_xchg(S.test_user, (int32_t)ranks.size(), ranks.data(), ns.data(), nr.data(), S.test_send.data(), S.test_recv.data()))
            return fail(-2, "test transport: the exchange callback failed");
        HIPC(hipMemcpyAsync(recv, S.test_recv.data(), tr * sizeof(double), hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));
        return 0;
    }
    size_t so = 0, ro = 0;
    NCCLC(ncclGroupStart());
    for (const MarchPeer &p : L.plan.peers) {
        const size_t ns = count(p.send_pos.size()), nr = count(p.recv_pos1.size());
        if (ns) NCCLC(ncclSend(send + so, ns, ncclDouble, p.rank, S.comm, st));
        if (nr) NCCLC(ncclRecv(recv + ro, nr, ncclDouble, p.rank, S.comm, st));
        so += ns; ro += nr;
    }
    NCCLC(ncclGroupEnd());
    return 0;
}

// The ring of one strip-major buffer (all nf fields of every halo cell) from the ranks that own the cells: pack + transfer on stream
// `st` (what is left is the unpack, incl. the duplicates).  Once per exchange pass for the state, once per call for the constants.
static int march_send_recv(double *buf, int nf, hipStream_t st)
{
    evp_launch_march_pack(buf, nf, B.send_pos, L.plan.n_send, B.cut_send, B.sendbuf, st);
    return ring_transfer(B.sendbuf, B.recvbuf, nf, st);
}

// One word that the ranks agree on (they must take the same path): the minimum (a vote: int32) or the maximum (a counter: uint32) over
// the ranks of the word at B.bad, into v; not `collective`: this rank's own word.  store: v goes to B.bad first -- otherwise a kernel
// has left the word there.  Over RCCL, or the test hook's reduce callback.
static int agree(unsigned &v, ncclRedOp_t op, bool store, bool collective)
{
    if (!B.bad && B.mem.alloc(B.bad, 1)) return -1;
    if (store) HIPC(hipMemcpyAsync(B.bad, &v, sizeof v, hipMemcpyHostToDevice, S.stream));
    if (collective && !S.test_reduce)
        NCCLC(ncclAllReduce(B.bad, B.bad, 1, op == ncclMax ? ncclUint32 : ncclInt32, op, S.comm, S.stream));
    HIPC(hipMemcpyAsync(&v, B.bad, sizeof v, hipMemcpyDeviceToHost, S.stream));
    HIPC(hipStreamSynchronize(S.stream));
    if (collective && S.test_reduce && S.test_reduce(S.test_user, op == ncclMax ? 1 : 0, &v))
        return fail(-2, "test transport: the reduce callback failed");
    return 0;
}
// ... the maximum over the ranks that have ring neighbours
static int agree_max(unsigned &v, bool store = false) { return agree(v, ncclMax, store, !L.plan.peers.empty() && S.d.nranks > 1); }

// ---- the ring without a communication library ------------------------------------------------------------------------
// What a rank tells each of its ring neighbours: how to map its inbox and where that neighbour's entries land in it.
struct MarchBlob {
    uint32_t magic, nf;
    int32_t from, to;
    uint64_t host_id;
    int64_t pid;
    uint64_t base, inbox_off, inbox_pstride, flag_off;      // bytes
    int64_t off_cells, count;                               // where the receiver of this blob writes, how many cells are expected
    hipIpcMemHandle_t handle;
};
constexpr int MARCH_BLOB_DOUBLES = 32;
static_assert(sizeof(MarchBlob) <= MARCH_BLOB_DOUBLES * sizeof(double), "MarchBlob must fit its slot");
constexpr uint32_t MARCH_BLOB_MAGIC = 0x4d524348u;      // "MRCH"

// Collective over the ranks of the ring (every rank with march neighbours runs it in the same call): inbox + flags in
// fine-grained memory, one blob per neighbour through the transport that is there anyway (RCCL send / recv, or the test
// hook), map, vote.  Any rank that cannot (another host, no IPC, switched off) makes everybody stay with the library.
static int march_direct_setup()
{
    State::March &M = S.march;
    M.direct = 0;
    const int np = (int)L.plan.peers.size();
    // Opt-in (CICE_EVP_HIP_MARCH_DIRECT=1), and only if every rank asks: on one GPU (the ring exchanged with the rank itself,
    // 450 x 2400 and 900 x 1200 pieces) it is no faster than RCCL -- 54.7 against 52.6 and 52.7 against 52.1 us per subcycle: the
    // pack kernel's uncached 8-byte stores take as long (13.4 us) as RCCL's pack + copy kernel (6.4 + 8.3) -- and what it does over
    // xGMI has never been measured; bench.py --gpus N times the 3600 x 2400 block this way too.
    {
        const bool want = march_direct_asked() &&
                          !(env("CICE_EVP_HIP_HALO") && !std::strcmp(env("CICE_EVP_HIP_HALO"), "rccl"));
        unsigned no = want ? 0u : 1u;
        if (agree_max(no, true)) return -1;
        if (no) {
            M.direct_why = want ? "not asked for on every rank" : "not asked for (CICE_EVP_HIP_MARCH_DIRECT=1)";
            return 0;
        }
    }
    bool ok = np > 0 && np <= EVP_MARCH_DIRECT_MAXPEER;
    if (!ok) M.direct_why = "more ring neighbours than the direct exchange holds";
    const size_t flag_bytes = (size_t)EVP_MARCH_DIRECT_MAXPEER * 64, count_off = flag_bytes, err_off = flag_bytes + 64;
    const size_t inbox_off = flag_bytes + 128;
    const size_t par_doubles = ((size_t)std::max(L.plan.n_recv, 1) * EVP_MARCH_S_NF + 31) & ~(size_t)31;
    std::vector<double> out((size_t)np * MARCH_BLOB_DOUBLES, 0.0), in((size_t)np * MARCH_BLOB_DOUBLES, 0.0);
    if (ok) {
        const size_t bytes = inbox_off + 2 * par_doubles * sizeof(double);
        if (B.mem.alloc_fine(B.dx_area, bytes)) {
            (void)hipGetLastError();
            g_err.clear();
            ok = false;
            M.direct_why = "no fine-grained device memory for the inbox";
        }
    }
    hipIpcMemHandle_t handle{};
    if (ok && hipIpcGetMemHandle(&handle, B.dx_area) != hipSuccess) {
        (void)hipGetLastError();
        ok = false;
        M.direct_why = "hipIpcGetMemHandle failed";
    }
    size_t ro = 0;
    for (int q = 0; q < np; ++q) {
        MarchBlob b{};
        b.magic = ok ? MARCH_BLOB_MAGIC : 0u;
        b.nf = EVP_MARCH_S_NF;
        b.from = S.d.rank; b.to = L.plan.peers[q].rank;
        b.host_id = host_identity();
        b.pid = (int64_t)getpid();
        b.base = (uint64_t)(uintptr_t)B.dx_area;
        b.inbox_off = inbox_off; b.inbox_pstride = par_doubles * sizeof(double); b.flag_off = (size_t)q * 64;
        b.off_cells = (int64_t)ro; b.count = (int64_t)L.plan.peers[q].recv_pos1.size();
        b.handle = handle;
        std::memcpy(&out[(size_t)q * MARCH_BLOB_DOUBLES], &b, sizeof b);
        ro += L.plan.peers[q].recv_pos1.size();
    }
    // the blobs travel like a ring of 32 doubles per neighbour
    {
        ScratchPool tmp;
        double *d_out = nullptr, *d_in = nullptr;
        if (tmp.upload(d_out, out) || tmp.alloc(d_in, in.size() + 1)) return -1;
        if (int rc = ring_transfer(d_out, d_in, MARCH_BLOB_DOUBLES, S.stream, false)) return rc;
        HIPC(hipMemcpyAsync(in.data(), d_in, in.size() * sizeof(double), hipMemcpyDeviceToHost, S.stream));
        HIPC(hipStreamSynchronize(S.stream));
    }
    EvpMarchDirect D{};
    D.npeers = np;
    for (int q = 0; q < np && ok; ++q) {
        MarchBlob b;
        std::memcpy(&b, &in[(size_t)q * MARCH_BLOB_DOUBLES], sizeof b);
        const MarchPeer &p = L.plan.peers[q];
        if (b.magic != MARCH_BLOB_MAGIC) { ok = false; M.direct_why = "rank " + std::to_string(p.rank) + " cannot take part"; break; }
        if (b.from != p.rank || b.to != S.d.rank || b.nf != EVP_MARCH_S_NF || b.count != (int64_t)p.send_pos.size()) {
            ok = false;
            M.direct_why = "rank " + std::to_string(p.rank) + " expects another ring from this rank than the plan sends";
            break;
        }
        if (b.host_id != host_identity()) { ok = false; M.direct_why = "rank " + std::to_string(p.rank) + " is on another host"; break; }
        char *base = nullptr;
        if (b.pid == (int64_t)getpid()) base = (char *)(uintptr_t)b.base;       // this very process (the ring exchanged with oneself)
        else {
            void *ptr = nullptr;
            if (hipIpcOpenMemHandle(&ptr, b.handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
                (void)hipGetLastError();
                ok = false;
                M.direct_why = "hipIpcOpenMemHandle failed for rank " + std::to_string(p.rank);
                break;
            }
            B.dx_mapped.push_back(ptr);
            base = (char *)ptr;
        }
        D.dst[q] = (double *)(base + b.inbox_off) + (size_t)b.off_cells * EVP_MARCH_S_NF;
        D.dst_pstride[q] = (size_t)(b.inbox_pstride / sizeof(double));
        D.peer_flag[q] = (unsigned *)(base + b.flag_off);
    }
    if (ok) {
        char *mine = (char *)B.dx_area;
        D.flags_in = (unsigned *)mine;
        D.count = (unsigned *)(mine + count_off);
        D.err = (int *)(mine + err_off);
        D.inbox = (const double *)(mine + inbox_off);
        D.inbox_pstride = par_doubles;
        D.timeout_ticks = (unsigned long long)(halo_timeout_ms() * 1.0e5);
        B.dx = D;
    }
    // everybody or nobody
    unsigned vote = ok ? 0u : 1u;
    if (agree_max(vote, true)) return -1;
    if (vote && ok) M.direct_why = "another rank cannot take part";
    M.direct = vote ? 0 : 2;         // 2: the first exchange runs both ways and compares
    verbose("rank %d: ring of the marching path %s%s", (int)S.d.rank,
            M.direct ? "as stores into the neighbours' HIP-IPC-mapped inboxes" : "through RCCL send / recv: ", M.direct ? "" : M.direct_why.c_str());
    return 0;
}

int march_direct_error()
{
    if (S.march.direct <= 0 || !B.dx.err) return 0;
    int e = 0;
    HIPC(hipMemcpy(&e, B.dx.err, sizeof e, hipMemcpyDeviceToHost));
    if (e) return fail(-8, "marching path: ring neighbour rank %d never signalled within the time-out (CICE_EVP_HIP_HALO_TIMEOUT_MS)",
                       (e - 1 < (int)L.plan.peers.size()) ? L.plan.peers[e - 1].rank : -1);
    return 0;
}

static int march_exchange(double *buf, double *buf2, int nf)
{
    if (L.plan.peers.empty()) return 0;
    State::March &M = S.march;
#ifndef CICE_EVP_HIP_TESTING
    // Product build: the ring goes through RCCL send / recv; its direct-store form is a switch of the test build (until a
    // multi-GPU node has ranked the two), so there is nothing to vote on -- and no collective that a rank without ring
    // neighbours would miss.
    M.direct = 0;
    M.direct_why = "test build only";
#else
    // Test build.  The switch is read at every state exchange and a change re-opens the set-up, which is COLLECTIVE over the
    // ranks that have ring neighbours (blobs, a vote): every such rank must see the same value at the same exchange -- the
    // tests and bench.py's ring_variants set it in all processes alike.  Mutually exclusive with CICE_EVP_HIP_MARCH_OVERLAP
    // (the overlapped path ignores it).
    if (nf == EVP_MARCH_S_NF) {
        const int asked = march_direct_asked() ? 1 : 0;
        if (M.direct >= 0 && asked != M.direct_asked) {       // (bench.py times one state both ways: the switch changed between two calls)
            HIPC(hipStreamSynchronize(S.stream));
            direct_close();
            M.direct = -1;
        }
        M.direct_asked = asked;
        if (M.direct < 0)
            if (int rc = march_direct_setup()) return rc;
    }
#endif
    if (nf == EVP_MARCH_S_NF && M.direct == 1) {
        const unsigned seq = ++B.dx_seq;
        evp_launch_march_pack_direct(buf, nf, B.send_pos, L.plan.n_send, B.cut_send, B.dx, seq, S.stream);
        evp_launch_march_unpack_direct(buf, buf2, nf, B.recv_pos1, B.recv_pos2, L.plan.n_recv, B.cut_recv, B.dx, seq, nullptr, nullptr, S.stream);
        return 0;
    }
    if (int rc = march_send_recv(buf, nf, S.stream)) return rc;
    evp_launch_march_unpack(buf, buf2, nf, B.recv_pos1, B.recv_pos2, L.plan.n_recv, B.cut_recv, B.recvbuf, S.stream);
    if (nf == EVP_MARCH_S_NF && M.direct == 2) {
        // once: the same ring through the inboxes as well, compared bit for bit with what the library delivered
        const unsigned seq = ++B.dx_seq;
        HIPC(hipMemsetAsync(B.bad, 0, sizeof(unsigned), S.stream));
        evp_launch_march_pack_direct(buf, nf, B.send_pos, L.plan.n_send, B.cut_send, B.dx, seq, S.stream);
        evp_launch_march_unpack_direct(buf, buf2, nf, B.recv_pos1, B.recv_pos2, L.plan.n_recv, B.cut_recv, B.dx, seq, B.recvbuf, B.bad, S.stream);
        unsigned bad = 0;
        if (agree_max(bad)) return -1;
        int e = 0;
        HIPC(hipMemcpy(&e, B.dx.err, sizeof e, hipMemcpyDeviceToHost));
        unsigned tmo = e ? 1u : 0u;
        if (agree_max(tmo, true)) return -1;
        if (e) HIPC(hipMemset(B.dx.err, 0, sizeof(int)));
        M.direct = (bad || tmo) ? 0 : 1;
        if (!M.direct) M.direct_why = tmo ? "a neighbour never signalled in the trial exchange" : "the trial exchange delivered other bits than the library";
        verbose("rank %d: trial of the direct ring exchange: %s", (int)S.d.rank, M.direct ? "identical to RCCL, in use from now on" : M.direct_why.c_str());
    }
    return 0;
}

static int march_exchange_mask()
{
    if (L.plan.peers.empty()) return 0;
    evp_launch_march_pack_mask(B.mask, B.send_midx, L.plan.n_send, B.sendbuf, S.stream);
    if (int rc = ring_transfer(B.sendbuf, B.recvbuf, 1, S.stream)) return rc;
    evp_launch_march_unpack_mask(B.mask, B.recv_midx, L.plan.n_recv, B.recvbuf, S.stream);
    return 0;
}

namespace {
struct TabBuilder {
    EvpMarchTab T{};
    void add(double *blk, double *pk, double *pk2, int nf, int slot)
    {
        T.blk[T.n] = blk; T.pk[T.n] = pk; T.pk2[T.n] = pk2; T.nf[T.n] = nf; T.slot[T.n] = slot; ++T.n;
    }
    // u, v and the 12 stresses of ping-pong copy `cur` of the block layout <-> slots 0 .. 13 of the state block(s)
    void add_state(int cur, double *pk, double *pk2 = nullptr)
    {
        add(S.u[cur], pk, pk2, EVP_MARCH_S_NF, 0);
        add(S.v[cur], pk, pk2, EVP_MARCH_S_NF, 1);
        for (int k = 0; k < 12; ++k) add(S.sig[cur][k], pk, pk2, EVP_MARCH_S_NF, 2 + k);
    }
};
}  // namespace

// Rows [y0, y1) of the rectangle as a window of the gather / scatter / check kernels: with the rows of the block arrays that hold
// an image of one of them (a cell of row j of block b lies on row blk_org[b].y + j - ilo).
static EvpMarchRows rows_window(int y0, int y1)
{
    const State::March &M = S.march;
    int j0 = 1 << 28, j1 = -(1 << 28);
    for (const MarchOrg &o : L.org) {
        j0 = std::min(j0, std::max(y0, -(1 << 20)) - o.y + M.G.ilo);
        j1 = std::max(j1, std::min(y1, 1 << 20) - o.y + M.G.ilo);
    }
    j0 = std::max(j0, 1);
    return EvpMarchRows{y0, y1, j0, std::max(j1 - j0, 0)};
}
// the rows the consistency checks look at: all of them, or -- under a fold band -- those the rectangle holds
static EvpMarchRows check_window()
{
    const State::March &M = S.march;
    return L.band_rows > 0 ? rows_window(-(1 << 28), M.G.nyr + EVP_MARCH_PAD) : EvpMarchAllRows;
}
// global rows [g0, g1) (march_plan.h: MarchFold) as a window of the rectangle this rank holds
static EvpMarchRows fold_window(int g0, int g1) { return rows_window(g0 - L.plan.me.gy0, g1 - L.plan.me.gy0); }

// The tile list of the fold band for the tile variant in use: every tile of every block that reaches row L.fold.list_row0 or above.
static int fold_tile_list(int variant, int *&list, int &count)
{
    auto it = B.fold_tiles.find(variant);
    if (it == B.fold_tiles.end()) {
        int tyb, gx, gy;
        evp_tile_geometry(S.max_ni, S.max_nj, variant, &tyb, &gx, &gy);
        MarchFold Fv = L.fold;
        Fv.trow = tyb - 1;
        std::vector<int> t;
        for (int b = 0; b < S.d.nblocks; ++b) {
            int by0, by1;
            march_fold_tile_rows(Fv, S.jglob0[b] - 1, S.jhi[b] - S.jlo[b] + 1, by0, by1);
            const int nbx = std::min(gx, (S.ihi[b] - S.ilo[b] + 1 + 62) / 63);
            for (int by = by0; by < std::min(by1, gy); ++by)
                for (int bx = 0; bx < nbx; ++bx) t.push_back((b * gy + by) * gx + bx);      // row-major tile id
        }
        int *dl = nullptr;
        if (B.mem.upload(dl, t)) return -1;
        it = B.fold_tiles.emplace(variant, std::make_pair(dl, (int)t.size())).first;
    }
    list = it->second.first;
    count = it->second.second;
    return 0;
}

// n subcycles of the fold band in the block layout, as enqueue_loop runs them on a tripole grid but over the band's tiles only.
// Several ranks: the velocity halo after each runs on EVERY rank, in lockstep, with the lists of the one-subcycle loop (its seam
// staging where the fold row is cut) -- a rank without band rows launches no tiles and only exchanges: what lands in its ghost cells
// is overwritten by the final scatter before anything reads it, and its ping-pong buffer flips with everybody else's.
static int fold_band_subcycles(int n, int &bcur, bool ends_call)
{
    const int variant = S.tyb % 100;         // (the list holds row-major tile ids)
    int *list = nullptr, count = 0;
    if (L.band_rows > 0)
        if (int rc = fold_tile_list(variant, list, count)) return rc;
    for (int k = 0; k < n; ++k) {
        if (count > 0) {
            EvpArgs A;
            fill_args(A, bcur, ends_call && k == n - 1);       // strintx/y, taubx/y of the band: from its own last subcycle
            A.tile_list = list; A.tile_count = count;
            evp_launch_subcycle(A, S.max_ni, S.max_nj, S.d.nblocks, variant, S.prm.strict != 0, cap_mode(), S.stream);
        }
        if (int rc = halo_uv(bcur ^ 1, true)) return rc;
        bcur ^= 1;
    }
    return 0;
}

// static fields into the constants block, once; are their ghost values images of one global field?
static int march_statics()
{
    State::March &M = S.march;
    TabBuilder G;
    double *src[5] = {S.stat[0], S.stat[1], S.hte, S.htn, S.stat[9]};
    const int slot[5] = {C_DXT, C_DYT, C_HTE, C_HTN, C_UAREAR};
    for (int k = 0; k < 5; ++k) G.add(src[k], B.cst, nullptr, EVP_MARCH_C_NF, slot[k]);
    evp_launch_march_gather(M.G, G.T, nullptr, nullptr, EvpMarchAllRows, S.stream);
    if (march_exchange(B.cst, nullptr, EVP_MARCH_C_NF)) return -1;      // (the per-call slots travel too: overwritten at every call)
    TabBuilder C;              // dxT dyT (fringe) | HTE HTN (fringe + column ilo-1 / row jlo-1)
    for (int k = 0; k < 4; ++k) C.add(src[k], B.cst, nullptr, EVP_MARCH_C_NF, slot[k]);
    HIPC(hipMemsetAsync(B.bad, 0, sizeof(unsigned), S.stream));
    evp_launch_march_check(M.G, C.T, nullptr, nullptr, 0, 2, B.bad, check_window(), S.stream);
    unsigned bad = 0;
    if (agree_max(bad)) return -1;
    M.stat_ok = bad == 0;
    M.stat_done = true;
    return 0;
}

// Decide once per init (after the first upload: EVP_F_METRICS is known then) whether this rank uses the path.
bool march_wanted()
{
    State::March &M = S.march;
    if (M.mode >= 0) return M.mode == 1;
    M.mode = 0;
    // a rank without blocks never gets here, so the agreement below would wait for it for ever: every rank sees it in the
    // global block table and stays off the path, without a vote
    if (S.d.nranks > 1 && !S.gtab[4].empty()) {
        std::vector<char> has((size_t)S.d.nranks, 0);
        for (int o : S.gtab[4])
            if (o >= 0 && o < S.d.nranks) has[(size_t)o] = 1;
        for (char h : has)
            if (!h) { M.why = "a rank holds no blocks"; return false; }
    }
    const int want = march_asked();
    // (a rank that was told CICE_EVP_HIP_MARCH=0 still takes part in the agreement below, voting no: an environment that
    // differs between the ranks then switches the path off everywhere instead of leaving the others in a collective)
    std::string why;
    bool ok = want != 0 && march_geometry(why);
    if (want == 0) why = "CICE_EVP_HIP_MARCH=0";
    if (S.d.nranks > 1 && (S.test_reduce || S.have_comm)) {
        // the choice must be the same on every rank (what decides it is partly local: e.g. whether the metric terms can be
        // recomputed from the edge lengths is verified on each rank's own cells); an agreement that fails switches the path off
        unsigned h = ok ? 1u : 0u;
        const bool fine = agree(h, ncclMin, true, true) == 0;
        g_err.clear();
        if (ok && (!fine || !h)) { ok = false; why = "another rank cannot use it"; }
    } else if (S.d.nranks > 1) {
        ok = false;
        if (why.empty()) why = "several ranks without an RCCL communicator";
    }
    if (!ok) {
        M.why = why;
        verbose("marching kernel off: %s", why.c_str());
        return false;
    }
    // worth it when the domain is far beyond what stays on the chip (the on-chip resident kernel is chosen before this
    // is asked): measured against the one-subcycle kernel 24 vs 26.5 us per subcycle at 389k cells, 39 vs 53 at 778k
    if (want < 0 && (long)S.d.nx_global * S.d.ny_global < 450000L * std::max(1, (int)S.d.nranks)) { M.why = "below 450k cells per rank"; return false; }
    // A fold band shared by several ranks: every band subcycle is a launch set and a collective halo on every piece, and the form has
    // not been timed against the one-subcycle kernels on these layouts -- so the size rule does not choose it yet.
    if (want < 0 && L.fold.H > 0 && S.d.nranks > 1) {
        M.why = "tripole grid on several ranks: marched zone + fold band runs when asked for (CICE_EVP_HIP_MARCH=1), not by the size rule";
        return false;
    }
    M.mode = 1;
    return true;
}

// does the kernel read the optional block (waterx watery TbU uvel_init vvel_init) under the flags in effect?
static bool need_opt(unsigned fl) { return !(fl & EVP_F_WATER_IS_OCN) || !(fl & EVP_F_TBU_ZERO) || S.prm.revp != 0.0; }

static void march_args(EvpMarch &A, int cur, int last)
{
    const State::March &M = S.march;
    const cice_evp_hip_params &q = S.prm;
    A.p = {q.arlx1i, q.denom1, q.brlx, q.revp, q.e_factor, q.epp2i, q.capping, q.Ktens, q.u0, q.cosw, q.sinw, q.rhow};
    A.deltaminEVP = q.deltaminEVP;
    A.nxr = M.G.nxr; A.nyr = M.G.nyr; A.ldx = M.G.ldx; A.own = M.G.own;
    A.nstrips = M.G.nstrips; A.nseg = L.nseg; A.seglen = L.seglen; A.nitems = L.nitems;
    A.wrapx = M.G.wrapx;
    A.last = last;
    A.kpass = L.kpass;
    A.order = env_int(env_test("CICE_EVP_HIP_MARCH_ORDER"), 1);
    A.flags = S.flags & S.flags_allowed;
    A.mask = B.mask;
    A.st_in = B.st[cur]; A.st_out = B.st[cur ^ 1];
    A.cst = B.cst;
    A.opt = need_opt(A.flags) ? B.opt : nullptr;
    A.diag = B.diag;
    A.dup = B.dup;
    A.items = nullptr;
}

// All ndte subcycles of a call.  Returns 0 when done (S.cur advanced like the one-subcycle loop would), < 0 on error.
int march_run(int ndte)
{
    State::March &M = S.march;
    if (march_alloc()) return -1;
    if (!M.stat_done && march_statics()) return -1;
    int cur = S.cur;
    int left = ndte;
    auto fallback = [&](const char *why) -> int {
        ++M.declined;
        M.why = why;
        verbose("marching kernel declined this call: %s", why);
        if (left > 0)
            if (int rc = enqueue_loop(left, cur)) return rc;
        S.cur = cur ^ (left & 1);
        return 0;
    };
    if (!M.stat_ok) return fallback("ghost values of the static grid fields are not images of one global field");
    // Several ranks: the redundant rim holds other ranks' cells and the optional operands travel in an exchange of their own -- both
    // only right where every rank formed the same verdicts on waterx / TbU, and those are per rank (evp_api.cpp: upload_impl).  Where
    // they differ this call goes through the one-subcycle kernel, on every rank.
    if (!L.plan.peers.empty() && S.d.nranks > 1) {
        unsigned hi = S.flags & S.flags_allowed & (EVP_F_WATER_IS_OCN | EVP_F_TBU_ZERO), lo = hi;
        if (agree(hi, ncclMax, true, true) || agree(lo, ncclMin, true, true)) return -1;
        if (hi != lo) return fallback("the ranks' verdicts on waterx == uocn / TbU == 0 differ");
    }
    // the passes of this call (march_plan.h: march_schedule); a single left-over subcycle goes first, through the one-subcycle
    // kernel in the block layout
    std::vector<MarchStep> steps = march_schedule(ndte, L.kpass, L.ring_valid, !L.plan.peers.empty(), L.fold.H > 0);
    if (!steps.empty() && steps[0].size == 1) {
        if (int rc = enqueue_loop(1, cur)) return rc;
        cur ^= 1;
        --left;
        S.cur = cur;     // the device state HAS advanced: an error further down must not leave S.cur on the old copy
        steps.erase(steps.begin());
    }
    M.call_passes = 0; M.call_subcycles = 0; M.call_band_subcycles = 0;
    if (left == 0) { S.cur = cur; return 0; }
    // Fold band (tripole grid): its subcycles flip the block layout's ping-pong buffers, one flip each; bcur names the buffer
    // that holds the band's current state.  The zone's rows reach it at the ring exchanges and in the final scatter.
    // Several ranks (shared): ONE band for the grid, held by the top row of ranks; every rank walks the same steps -- the band's
    // per-subcycle halo is collective -- whether it holds band rows (band) or not.
    const bool fold = L.fold.H > 0, band = L.band_rows > 0, shared = fold && S.d.nranks > 1;
    int bcur = cur;
    const unsigned fl = S.flags & S.flags_allowed;
    // ---- gather the state and the per-call inputs ----
    {
        TabBuilder G;
        G.add_state(cur, B.st[0], B.st[1]);
        G.add(S.in[F_STRENGTH], B.cst, nullptr, EVP_MARCH_C_NF, C_STRENGTH);
        G.add(S.vrelfac, B.cst, nullptr, EVP_MARCH_C_NF, C_VRELFAC);
        G.add(S.in[F_UOCN], B.cst, nullptr, EVP_MARCH_C_NF, C_UOCN); G.add(S.in[F_VOCN], B.cst, nullptr, EVP_MARCH_C_NF, C_VOCN);
        G.add(S.in[F_FORCEX], B.cst, nullptr, EVP_MARCH_C_NF, C_FORCEX); G.add(S.in[F_FORCEY], B.cst, nullptr, EVP_MARCH_C_NF, C_FORCEY);
        G.add(S.in[F_UMASSDTI], B.cst, nullptr, EVP_MARCH_C_NF, C_UMASSDTI); G.add(S.in[F_FM], B.cst, nullptr, EVP_MARCH_C_NF, C_FM);
        if (!(fl & EVP_F_WATER_IS_OCN)) {
            G.add(S.in[F_WATERX], B.opt, nullptr, EVP_MARCH_O_NF, O_WATERX); G.add(S.in[F_WATERY], B.opt, nullptr, EVP_MARCH_O_NF, O_WATERY);
        }
        if (!(fl & EVP_F_TBU_ZERO)) G.add(S.in[F_TBU], B.opt, nullptr, EVP_MARCH_O_NF, O_TBU);
        if (S.prm.revp != 0.0) {
            G.add(S.in[F_UVEL_INIT], B.opt, nullptr, EVP_MARCH_O_NF, O_UINIT); G.add(S.in[F_VVEL_INIT], B.opt, nullptr, EVP_MARCH_O_NF, O_VINIT);
        }
        evp_launch_march_gather(M.G, G.T, S.mask, B.mask, EvpMarchAllRows, S.stream);
        // the two-cell ring of everything: other ranks' cells (once per call for the constants and the mask)
        if (march_exchange(B.cst, nullptr, EVP_MARCH_C_NF)) return -1;
        if (need_opt(fl) && march_exchange(B.opt, nullptr, EVP_MARCH_O_NF)) return -1;
        if (march_exchange_mask()) return -1;
        if (march_exchange(B.st[0], B.st[1], EVP_MARCH_S_NF)) return -1;
    }
    if (M.checked_seq != S.upload_seq || !L.plan.peers.empty()) {
        // first call on this uploaded state: are the caller's ghost values images of one global state?
        TabBuilder C;
        C.add_state(cur, B.st[0]);
        C.add(S.in[F_STRENGTH], B.cst, nullptr, EVP_MARCH_C_NF, C_STRENGTH);
        HIPC(hipMemsetAsync(B.bad, 0, sizeof(unsigned), S.stream));
        evp_launch_march_check(M.G, C.T, S.mask, B.mask, 2, 13, B.bad, check_window(), S.stream);
        unsigned bad = 0;
        if (agree_max(bad)) return -1;
        if (bad) return fallback("ghost cells of the uploaded state are not images of one global state (here or on another rank)");
        M.checked_seq = S.upload_seq;
    }
    // ---- the passes ----
    // Exchange passes (the redundant rim and the ring have been used up; the last): the (strip, row) units that hold cells other
    // ranks are waiting for are advanced FIRST, by an early launch of the same kernel over short segments on the second stream;
    // their pack and the RCCL send / recv follow there while the rest of the pass -- every other (strip, row), rest_items -- runs
    // on the compute stream: the transfer is overlapped with the interior of the pass instead of following it (ice_HaloUpdate ->
    // RCCL point-to-point on a second HIP stream over interior compute).  The two launches read the same input state and store
    // into disjoint cells (a cell's result does not depend on the segment it is computed in).  Only the unpack waits for the
    // pass: the pass still writes its (spent) redundant rim where the received cells go.
    const int npass = (int)steps.size();
    int rc = 0;
    // Opt-in, in the PRODUCT library too (CICE_EVP_HIP_MARCH_OVERLAP=1; every rank alike): where it can be measured -- one GPU, the
    // ring exchanged with the rank itself, profiles/r06_ring_rank.txt -- it still loses, 64.2 against 57.3 us per subcycle on the
    // 450 x 2400 piece and 61.2 against 56.9 on 900 x 1200, although the two launches no longer advance the band twice (rounds 4-5:
    // 57.7 against 51.2): the pass is bound by instruction issue with every SIMD holding one wave for the whole pass, so there is
    // no idle resource to hide a transfer under, and "early" means SHORT segments for the band -- 2K - 1 rows of warm-up on 7 stored.
    // On one GPU the transfer is a 7-us device copy; over xGMI it is 1.6 MB per neighbour every eighth subcycle, and only a node
    // can say whether hiding that is worth 6 us per subcycle.  bench.py --gpus N --extras ring_variants times both.
    // (beside a fold band on several ranks the serial form is taken: the band's rows must be in the rectangle before the ring travels)
    const bool overlap = !L.plan.peers.empty() && !L.band_items.empty() && M.direct != 1 && march_overlap_asked() && !march_direct_asked() && !shared;
    for (const MarchStep &step : steps) {
        // step.exch: the ring of the new state travels after this pass -- the next one needs more valid cells than are left, or this
        // is the last one (the way back to the block layout reads the ghost cells from it)
        // step.fexch: the fold band's ring, at the same points but not after the last pass -- the final scatter moves the zone's rows then
        const bool exch = step.exch;
        EvpMarch A;
        march_args(A, rc, step.last);
        A.kpass = step.size;
        if (exch && overlap) {
            HIPC(hipEventRecord(B.ev_in, S.stream));
            HIPC(hipStreamWaitEvent(S.stream_comm, B.ev_in, 0));
            EvpMarch E = A;
            E.items = B.band_items;
            E.nitems = (int)L.band_items.size();           // (the last pass: the band's diagnostics are this launch's business)
            evp_launch_march(E, S.prm.strict != 0, cap_mode(), S.stream_comm);
            if (int e = march_send_recv(B.st[rc ^ 1], EVP_MARCH_S_NF, S.stream_comm)) return e;
            A.items = B.rest_items;                              // the pass itself: everything else
            A.nitems = (int)L.rest_items.size();
        }
        if (A.nitems > 0) evp_launch_march(A, S.prm.strict != 0, cap_mode(), S.stream);
        rc ^= 1;
        if (exch && overlap) {
            HIPC(hipEventRecord(B.ev_main, S.stream));
            HIPC(hipStreamWaitEvent(S.stream_comm, B.ev_main, 0));
            evp_launch_march_unpack(B.st[rc], nullptr, EVP_MARCH_S_NF, B.recv_pos1, B.recv_pos2, L.plan.n_recv, B.cut_recv, B.recvbuf, S.stream_comm);
            HIPC(hipEventRecord(B.ev_done, S.stream_comm));
            HIPC(hipStreamWaitEvent(S.stream, B.ev_done, 0));
        } else if (exch && !shared) {
            if (march_exchange(B.st[rc], nullptr, EVP_MARCH_S_NF)) return -1;
        }
        if (shared) {
            // The same steps with the rank ring BETWEEN the two halves of the trade.  The band catches up; on the ranks that hold band
            // rows, the band's ext + P rows above the zone go into the rectangle; then the ring of the rectangle travels -- the corner
            // cells above the zone from the rows that gather has just filled on the rank that owns them; only then do the zone's
            // ext + P rows under the band go into the block layout.  Every image of a cell: at a rank's x-edges the ghost columns and
            // the T-cells of the east fringe are its neighbour's zone cells, and the ring has just brought them.  (Before the ring they
            // would come out of spent ring cells; a velocity halo afterwards would mend the velocities but not the fringe stresses,
            // which every block carries for itself from one subcycle to the next.)
            if (int e = fold_band_subcycles(step.size, bcur, step.last)) return e;
            if (band) M.call_band_subcycles += step.size;
            TabBuilder T;
            T.add_state(bcur, B.st[rc]);
            if (step.fexch && band)
                evp_launch_march_gather(M.G, T.T, nullptr, nullptr, fold_window(L.fold.to_rect[0], L.fold.to_rect[1]), S.stream);
            if (exch && march_exchange(B.st[rc], nullptr, EVP_MARCH_S_NF)) return -1;
            if (step.fexch && band)
                evp_launch_march_scatter(M.G, T.T, S.mask, 2, 12, fold_window(L.fold.to_block[0], L.fold.to_block[1]), S.stream);
        } else if (fold) {
            // the band catches up with the pass; then, when either side has used up its ring, the two trade rows: the zone's
            // ext + P rows under the band into the block layout (every image of a cell), the band's ext + P rows above the zone
            // into the rectangle (every lane that holds the column)
            if (int e = fold_band_subcycles(step.size, bcur, step.last)) return e;
            M.call_band_subcycles += step.size;
            if (step.fexch) {
                TabBuilder T;
                T.add_state(bcur, B.st[rc]);
                evp_launch_march_scatter(M.G, T.T, S.mask, 2, 12, rows_window(L.fold.to_block[0], L.fold.to_block[1]), S.stream);
                evp_launch_march_gather(M.G, T.T, nullptr, nullptr, rows_window(L.fold.to_rect[0], L.fold.to_rect[1]), S.stream);
            }
        }
    }
    HIPC(hipGetLastError());
    M.passes += npass;
    M.subcycles += left;
    M.call_passes = npass; M.call_subcycles = left;
    // ---- back to the block layout ----
    {
        // (a fold band: into the buffer its last subcycle wrote, the zone's rows only -- the band's own are current there)
        TabBuilder T;
        T.add_state(bcur, B.st[rc]);
        T.add(S.in[F_STRINTX], B.diag, nullptr, EVP_MARCH_D_NF, 0); T.add(S.in[F_STRINTY], B.diag, nullptr, EVP_MARCH_D_NF, 1);
        T.add(S.in[F_TAUBX], B.diag, nullptr, EVP_MARCH_D_NF, 2); T.add(S.in[F_TAUBY], B.diag, nullptr, EVP_MARCH_D_NF, 3);
        evp_launch_march_scatter(M.G, T.T, S.mask, 2, 12, band ? fold_window(-(1 << 27), L.fold.zone) : EvpMarchAllRows, S.stream);
    }
    HIPC(hipGetLastError());
    S.cur = bcur;           // without a band the passes leave the block layout's ping-pong buffer where it was: the scatter wrote the
                            // new state there; the band's subcycles flipped it once each
    return 0;
}

}  // namespace evp_host

#ifdef CICE_EVP_HIP_TESTING
extern "C" int cice_evp_hip_set_test_transport(cice_evp_hip_test_xchg_fn xchg, cice_evp_hip_test_reduce_fn reduce, void *user)
{
    using namespace evp_host;
    if ((xchg == nullptr) != (reduce == nullptr)) return fail(-1, "test transport: give both callbacks or none");
    S.test_xchg = xchg; S.test_reduce = reduce; S.test_user = user;
    return 0;
}

// Host-only: the plan of dims->rank without touching a device (CPU tests).
extern "C" int cice_evp_hip_march_plan(const cice_evp_hip_dims *dims, int32_t own_max, int32_t wrap_inside, int32_t ext, int32_t *geo14,
                                       int32_t *peer_rank, int32_t *peer_nsend, int32_t *peer_nrecv, int32_t *send_pos,
                                       int32_t *recv_pos1, int32_t *recv_pos2)
{
    using namespace evp_host;
    if (!dims) return fail(-1, "null dims");
    MarchPlan P;
    if (!build_march_plan(*dims, own_max > 0 ? own_max : EVP_MARCH_OWN, wrap_inside != 0, ext, P)) return fail(-3, "march plan: %s", P.error.c_str());
    if (geo14) {
        const int32_t g[14] = {P.me.gx0, P.me.gy0, P.me.nxr, P.me.nyr, P.me.own, P.me.nstrips, (int32_t)P.peers.size(), P.n_send,
                               P.n_recv, P.wrapx ? 1 : 0, P.ext_w, P.ext_e, P.ext_s, P.ext_n};
        for (int k = 0; k < 14; ++k) geo14[k] = g[k];
    }
    size_t so = 0, ro = 0;
    for (size_t q = 0; q < P.peers.size(); ++q) {
        const MarchPeer &p = P.peers[q];
        if (peer_rank) peer_rank[q] = p.rank;
        if (peer_nsend) peer_nsend[q] = (int32_t)p.send_pos.size();
        if (peer_nrecv) peer_nrecv[q] = (int32_t)p.recv_pos1.size();
        for (size_t k = 0; k < p.send_pos.size(); ++k)
            if (send_pos) send_pos[so + k] = p.send_pos[k];
        for (size_t k = 0; k < p.recv_pos1.size(); ++k) {
            if (recv_pos1) recv_pos1[ro + k] = p.recv_pos1[k];
            if (recv_pos2) recv_pos2[ro + k] = p.recv_pos2[k];
        }
        so += p.send_pos.size(); ro += p.recv_pos1.size();
    }
    return 0;
}

// Host-only: the whole layout of dims->rank as the host would build it when asked `ask7` (march_plan.h: build_march_layout).
extern "C" int cice_evp_hip_march_layout(const cice_evp_hip_dims *dims, const int32_t *ask7, int32_t *info37, int32_t *blkid, int32_t *org2,
                                         uint32_t *dup, int32_t *ring5, int32_t *cuts3, int32_t *band4, int32_t *rest4)
{
    using namespace evp_host;
    if (!dims || !ask7) return fail(-1, "null dims / ask");
    MarchAsk a;
    a.own_max = ask7[0]; a.wrap_inside = ask7[1] != 0; a.ext = ask7[2]; a.kpass = ask7[3]; a.seglen = ask7[4]; a.bandseg = ask7[5]; a.tyb = ask7[6];
    MarchLayout Y;
    if (!build_march_layout(*dims, a, Y)) return fail(-3, "march layout: %s", Y.why.c_str());
    const int np = (int)Y.plan.peers.size(), ns = Y.plan.n_send, nr = Y.plan.n_recv;
    if (info37) {
        const MarchPlan &P = Y.plan;
        const int32_t v[37] = {Y.ext, Y.ring_valid, Y.kpass, Y.bsx, Y.bsy, Y.nbx, Y.nby, P.me.nxr, P.me.nyr, Y.ldx, Y.rows, P.me.own, P.me.nstrips, P.wrapx,
                               P.me.gx0, P.me.gy0, P.ext_w, P.ext_s, P.owned.nxr, P.owned.nyr, P.owned.nyr + Y.band_rows, (int32_t)Y.nblk, Y.seglen, Y.nseg, Y.nitems, np, ns, nr,
                               (int32_t)Y.band_items.size(), (int32_t)Y.rest_items.size(), Y.fold.H, Y.fold.zone, (int32_t)Y.org.size(),
                               (int32_t)Y.dup.size(), Y.band_rows, Y.band_ranks, Y.fold.list_row0};
        std::copy(v, v + 37, info37);
    }
    if (blkid) std::copy(Y.blkid.begin(), Y.blkid.end(), blkid);
    if (org2) std::memcpy(org2, Y.org.data(), Y.org.size() * sizeof(MarchOrg));
    if (dup) std::copy(Y.dup.begin(), Y.dup.end(), dup);
    if (ring5 && !Y.send_pos.empty()) {      // send_pos, send_midx [n_send] | recv_pos1, recv_pos2, recv_midx [n_recv]
        int32_t *o = ring5;
        for (const std::vector<int32_t> *l : {&Y.send_pos, &Y.send_midx, &Y.recv_pos1, &Y.recv_pos2, &Y.recv_midx}) o = std::copy(l->begin(), l->end(), o);
    }
    if (cuts3) {           // where each peer's share begins in the send / the receive list | the peers' ranks (and -1)
        std::copy(Y.cut_send, Y.cut_send + np + 1, cuts3);
        std::copy(Y.cut_recv, Y.cut_recv + np + 1, cuts3 + np + 1);
        for (int q = 0; q <= np; ++q) cuts3[2 * (np + 1) + q] = q < np ? Y.plan.peers[q].rank : -1;
    }
    if (band4) std::memcpy(band4, Y.band_items.data(), Y.band_items.size() * sizeof(MarchItem));
    if (rest4) std::memcpy(rest4, Y.rest_items.data(), Y.rest_items.size() * sizeof(MarchItem));
    return 0;
}

// Host-only: the passes of a call of ndte subcycles (march_plan.h: march_schedule); steps4 = per step {size, exch, fexch, last}.
extern "C" int cice_evp_hip_march_schedule(int32_t ndte, int32_t kpass, int32_t ring_valid, int32_t has_peers, int32_t fold, int32_t *n, int32_t *steps4)
{
    const std::vector<MarchStep> st = march_schedule(ndte, kpass, ring_valid, has_peers != 0, fold != 0);
    if (n) *n = (int32_t)st.size();
    for (size_t k = 0; steps4 && k < st.size(); ++k) {
        const int32_t v[4] = {st[k].size, st[k].exch, st[k].fexch, st[k].last};
        std::copy(v, v + 4, steps4 + 4 * k);
    }
    return 0;
}

// Host-only: how a tripole grid on one rank is shared between the marched zone and the fold band (march_plan.h: MarchFold).
extern "C" int cice_evp_hip_march_fold_plan(const cice_evp_hip_dims *dims, int32_t ext, int32_t tyb, int32_t *out10, int32_t *tile_rows)
{
    using namespace evp_host;
    if (!dims) return fail(-1, "null dims");
    MarchFold F;
    if (!build_march_fold(*dims, ext, tyb, F)) return fail(-3, "march fold plan: %s", F.error.c_str());
    MarchPlan P;
    if (!build_march_plan(*dims, EVP_MARCH_OWN, true, ext, P, F.H)) return fail(-3, "march fold plan: %s", P.error.c_str());
    if (out10) {
        const int32_t v[10] = {F.zone, F.H, F.ext, F.trow, F.list_row0, F.to_block[0], F.to_block[1], F.to_rect[0], F.to_rect[1], P.me.nyr};
        for (int k = 0; k < 10; ++k) out10[k] = v[k];
    }
    for (int b = 0; tile_rows && b < dims->nblocks; ++b) {
        int by0, by1;
        march_fold_tile_rows(F, dims->jglob0[b] - 1, dims->jhi[b] - dims->jlo[b] + 1, by0, by1);
        tile_rows[2 * b] = by0; tile_rows[2 * b + 1] = by1;
    }
    return 0;
}
#endif  // CICE_EVP_HIP_TESTING
