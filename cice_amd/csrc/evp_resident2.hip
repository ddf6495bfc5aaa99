// =====================================================================
// On-chip resident EVP subcycle: tagged hand-off.
//
// (A first generation, retired in round 5, published a tile's velocities and then a flag; the
// neighbours polled the flag, passed a barrier and only then loaded the velocities: per subcycle
// one store drain, one flag round trip and one data round trip sat on the critical path,
// ~55 % of its time by shader-clock stamps.)  Here the data IS the flag: a velocity that another tile needs is published as one aligned 16-byte granule
//      { tag, value.lo, value.hi, tag }        tag = launch epoch | subcycle
// written by ONE write-through (sc1) dwordx4 store; the reader re-reads the granule
// (sc1, L1-bypassing) until both tags carry the subcycle it waits for -- a torn
// granule cannot pass (MI355X_MICROARCH.md, "R2": observed untorn, checked anyway).
// No flags, no store drain, no fences.  Velocities used inside the tile never leave
// the CU: they live in an LDS tile with a one-cell ring; only the ring is polled
// (<= 2(W+H) threads, one granule pair each).  Records are double-buffered by subcycle
// parity; a tile can be at most one subcycle ahead of a neighbour, so two suffice.
//
// Same arithmetic and ownership rules as the streaming kernel => same bits.  Every spin is bounded and raises the error word.
//
// Rim wave / interior waves (PERM, the 16 x 16 tile).  A subcycle of a tile is a dependent chain:
// (tripoleT, round 6: a top-row U-cell is the image of a cell of row NY-1; it takes -1 x that cell's new value after its own momentum
// step, through the record that cell publishes -- EvpResident2::tfold, the seam table names the source)
// neighbours publish -> ring poll -> stress -> barrier -> momentum step -> publish.  Only the T-cells
// on the rim of the tile read ring velocities (60 of 256 in a full 16 x 16 tile), and the ring has
// at most 64 entries: a host-built permutation puts those T-cells -- and the ring poll -- into
// wave 0, all other T-cells into waves 1-3.  Waves 1-3 start their stress update straight after the
// barrier that ends the previous momentum step, from velocities that never left the CU, while wave 0
// waits for the neighbours' records: the hand-off latency (about 1 us of the 5.5 us a subcycle took
// on gx1, three tiles per CU time-sharing the SIMDs) overlaps with three quarters of the tile's
// arithmetic instead of preceding all of it.  The lane -> cell map is arbitrary here because no
// array access of the loop is a global one; the eight stress-divergence partials travel through LDS
// by cell position.  Same arithmetic per cell => same bits.
//
// RIMU (the lean variant's schedule where the lane tables allow it: rim_plan.h).  Under the schedule above every wave meets at a
// barrier B1 between the stress update and the momentum step, because the U-cells that read a rim T-cell's partials -- the edge
// U-cells, which are also the ones that write records -- are scattered over all four waves; the interior waves then sit at B1
// for 45 % of a subcycle and step inside the chain's window.  Here the rim wave (chunk 0) holds L_T (the rim T-cells, and in a
// full tile the four depth-1 corner cells) AND L_U (every U-cell that reads a partial of L_T or writes a record); every other
// U-cell stays with its T-cell's lane in an interior wave (chunks 1-3).  By the closure of L_U no U-cell outside L_U reads a
// T-cell of L_T, and no T-cell of L_T reads the velocity of a U-cell outside L_U.  Per subcycle k:
//   interior wave:  stress of its T-cells -> partials to the planes -> s_waitcnt lgkmcnt(0) -> slot[chunk - 1] = k + 1 ->
//                   spin until all three slots >= k + 1 -> momentum step of its U-cells -> s_u / s_v -> barrier B2
//   rim wave:       ring poll -> stress of L_T -> planes -> spin on the three slots -> second part of the momentum step of L_U
//                   -> records -> s_u / s_v -> barrier B2 -> first part of the momentum step of subcycle k + 1
//                   (stepu_pre_cell: reads the cell's own new velocity and per-call operands only)
// Who writes and who reads what, between which two synchronisation points (B2(k): the barrier that ends subcycle k):
//   s_u / s_v, ring cells       written by the rim wave after its poll of subcycle k, read by L_T only (rim wave, program order;
//                               LDS operations of one wave complete in order).  Interior T-cells read no polled ring cell.
//   s_u / s_v, cells of L_U     written by the rim wave AFTER its slot spin of subcycle k, i.e. after every interior wave has
//                               finished the stress update of subcycle k (its last read of them before B2(k)); read by L_T in
//                               subcycle k + 1 (same wave) and by interior T-cells after B2(k).
//   s_u / s_v, other U-cells    written by their interior wave after ITS slot spin of subcycle k: every interior wave's stress
//                               reads of subcycle k are complete, and the rim wave never reads them; read after B2(k).
//   planes, interior T-cells    (all eight: the NE partials str[0] / str[4] of a T-cell travel too, its own U-cell may sit on
//                               another lane) written before the wave's slot says k + 1, read by interior U-cells and by L_U
//                               only after the reader has seen all three slots >= k + 1; written again only after B2(k), which
//                               no reader passes before its reads.  A position without an ice T-cell is never written: the
//                               planes are zeroed once, before the loop.
//   planes, cells of L_T        written and read by the rim wave only, in program order.
//   slots                       slot[q] = k + 1 is written once per subcycle by lane 0 of interior wave q after its planes are
//                               complete, and read (volatile, workgroup scope) by every wave; it only grows, and subcycle k + 1's
//                               value is written after B2(k), when nobody spins on k + 1 any more.  Zeroed before the loop.
// One workgroup barrier per subcycle remains.  Every spin is bounded; a wave whose wait gives up sets s_bad and goes straight to
// B2, after which every wave tests s_bad and the workgroup leaves together (err[0] == 5: the slot spin).  Two record buffers
// still suffice: publishing and polling are as independent of the ice masks as before (every cell another tile mirrors is in L_U
// and stores its record every subcycle, every ring entry with a producer is polled every subcycle), and a tile's records of
// subcycle k + 1 are stored by the wave that polled all of its ring entries of subcycle k before, in program order -- a tile
// cannot be more than one subcycle ahead of any tile that still has to read its records.
// =====================================================================
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <type_traits>

// Debug hooks (lagging tiles, a workgroup that never shows up, A/B switches) and the per-phase cycle stamps exist in the
// TEST build's object of this file only (-DCICE_EVP_HIP_TESTING, linked into libcice_evp_hip_testing.so): the product
// kernel does not test R.dbg / R.prof at all.
#ifdef CICE_EVP_HIP_TESTING
#define RES_DBG(R) ((R).dbg)
#define RES_PROF(R) ((R).prof != nullptr)
#else
#define RES_DBG(R) 0
#define RES_PROF(R) false
#endif

#include "evp_math.h"

namespace {

constexpr int RTY = 4;   // waves per workgroup (one per SIMD)

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// two adjacent granules (u then v) of one cell, write-through / L1-bypassing
__device__ __forceinline__ void st_rec2(void *p, v4u a, v4u b)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\tglobal_store_dwordx4 %0, %2, off offset:16 sc1"
                 :
                 : "v"(p), "v"(a), "v"(b)
                 : "memory");
}
__device__ __forceinline__ void ld_rec2(const void *p, v4u &a, v4u &b)
{
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b)
                 : "v"(p)
                 : "memory");
}
// the same as scalar base + 32-bit lane offset (the saddr form: no 64-bit address arithmetic per lane)
__device__ __forceinline__ void st_rec2_s(const void *base, unsigned off, v4u a, v4u b)
{
    asm volatile("global_store_dwordx4 %0, %1, %3 sc1\n\tglobal_store_dwordx4 %0, %2, %3 offset:16 sc1"
                 :
                 : "v"(off), "v"(a), "v"(b), "s"(base)
                 : "memory");
}
__device__ __forceinline__ void ld_rec2_s(const void *base, unsigned off, v4u &a, v4u &b)
{
    asm volatile("global_load_dwordx4 %0, %2, %3 sc1\n\tglobal_load_dwordx4 %1, %2, %3 offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b)
                 : "v"(off), "s"(base)
                 : "memory");
}
// the same at system scope: records another GPU writes into this one's buffer / this one into a peer's
__device__ __forceinline__ void st_rec2_sys(void *p, v4u a, v4u b)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\tglobal_store_dwordx4 %0, %2, off offset:16 sc0 sc1"
                 :
                 : "v"(p), "v"(a), "v"(b)
                 : "memory");
}
__device__ __forceinline__ void ld_rec2_sys(const void *p, v4u &a, v4u &b)
{
    asm volatile("global_load_dwordx4 %0, %2, off sc0 sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc0 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b)
                 : "v"(p)
                 : "memory");
}
__device__ __forceinline__ v4u pack_rec(double x, unsigned tag)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    v4u r;
    r.x = tag; r.y = (unsigned)bits; r.z = (unsigned)(bits >> 32); r.w = tag;
    return r;
}
__device__ __forceinline__ double unpack_rec(v4u r)
{
    return __longlong_as_double((long long)(((unsigned long long)r.z << 32) | r.y));
}

// quad permute of a double (one DPP move per 32-bit half): lane l of every four adjacent lanes reads lane (l ^ X)
template <int CTRL>
__device__ __forceinline__ double quad_perm(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
constexpr int QP_X1 = 0xB1, QP_X2 = 0x4E, QP_X3 = 0x1B;      // quad_perm [1,0,3,2], [2,3,0,1], [3,2,1,0]

// REMOTE: some ghost cells mirror cells of OTHER ranks (GPUs of the same node).  Their records
// live in this rank's record buffer and are written by the producing GPU with plain 16-byte
// stores over xGMI (the buffer is mapped there through HIP IPC); an edge cell with remote images
// stores its record into the peers' buffers as well.  Nothing else changes: the halo exchange is
// a remote store plus the ring poll that is there anyway.
// COOP (16 x 16 tiles, strict arithmetic, the default scalars -- CAP == 3 -- only): the T-cells that read ring velocities are
// not updated by one thread each after the ring poll -- 700 instructions of one wave on the critical path of every
// subcycle, while the other three waves of the tile wait at the barrier -- but by FOUR lanes each, one per corner, spread over
// all four waves: a lane works out the strain rates, Delta, the viscosities and the three stresses of its corner (the corner's
// operands and signs selected per lane, the operations and their order those of stress_cell: a - b*c == a + (-b)*c, x + y == y + x
// bit for bit), fetches the other three corners' stresses with quad-permute moves, and forms the two stress-divergence partials
// that carry its corner's coefficients.  The cell's stresses live three per lane in those quads for the whole call.
// LEAN (one rank and block, no fold, TbU == 0, water == ocean current, revp == 0; res2_choose, res2_variant.cpp): none of the code for
// the other cases is in the subcycle loop, which runs two subcycles per trip (one per record buffer), the record loads and stores
// addressed as scalar buffer base + lane offset.  Same operations in the same order => same bits
// (profiles/r07_resident_lean_*.txt, tools/resident_isa_mix.py).
// RIMU: the lean loop on the rim-wave schedule of the header (profiles/r14_resident_rim_u.txt); where a tile's lane tables cannot
// satisfy rim_plan.h's rules the launch takes the lean loop as it was (per launch, evp_host_resident.cpp).
// Range-proved arithmetic (the two lean loops; evp_range_math.h, profiles/r15_resident_range_math.txt): a wave whose active lanes
// all have their operands inside a window of exponents takes the cores of the fp64 square root and division without the range
// handling the compiler wraps them in, any other wave the compiler's forms -- per pass, a uniform branch, the same bits.  The
// product compiles it in or out (EVP_RES2_RANGE_DEFAULT); the test build carries it with a switch (EVP_RES2_HOOK_NO_RANGE: always the
// compiler's forms; CICE_EVP_HIP_RES_RANGE=0 sets it).
template <bool STRICT, int CAP, int LOGW, bool REMOTE, bool COOP = false, bool LEAN = false, bool RIMU = false>
__global__ __launch_bounds__(64 * RTY, REMOTE ? 2 : 3) void evp_resident2_tile(EvpArgs A, EvpResident2 R)
{
    static_assert(!COOP || (STRICT && CAP == 3 && LOGW == 4), "COOP: 16 x 16 tiles, strict build, default scalars");
    static_assert(!LEAN || (!REMOTE && !COOP && LOGW == 4), "LEAN: one rank, 16 x 16 tiles, one thread per rim cell");
    static_assert(!RIMU || LEAN, "RIMU: a schedule of the lean loop");
    using MM = Math<STRICT>;
#ifdef CICE_EVP_HIP_TESTING
    constexpr bool RANGE = LEAN;
#else
    constexpr bool RANGE = LEAN && EVP_RES2_RANGE_DEFAULT;
#endif
    // the policy of the lean loops' arithmetic; POLE: the same with taubx / tauby formed every subcycle (the first lean loop)
    // SPLIT (the rim-wave schedule): the U-cell's two divisions on the cores, their reciprocal formed in the first part of the
    // momentum step, which the rim wave runs off the hand-off chain (EVP_RES2_SPLITDIV_DEFAULT; the test build carries it with a
    // switch, EVP_RES2_HOOK_SPLITDIV, CICE_EVP_HIP_RES_SPLITDIV)
#ifdef CICE_EVP_HIP_TESTING
    constexpr bool SPLIT = true;
#else
    constexpr bool SPLIT = EVP_RES2_SPLITDIV_DEFAULT != 0;
#endif
    using POLR = std::conditional_t<SPLIT, evp_range::RangeMathLazySplit, evp_range::RangeMathLazy>;
    using POL = std::conditional_t<RANGE, std::conditional_t<RIMU, POLR, evp_range::RangeMath>, evp_range::LibMath>;
    using POLE = std::conditional_t<RANGE, evp_range::RangeMath, evp_range::LibMath>;
    constexpr int W = 1 << LOGW;
    constexpr int H = 256 / W;
    constexpr int LW = W + 1;                 // LDS velocity tile: (H+1) x (W+1), origin (-1,-1)
    constexpr int NUV = ((H + 1) * LW + 7) & ~7;
    constexpr bool PERM = (LOGW == 4);        // rim wave / interior waves (see the header)
    constexpr int NSTR = RIMU ? 8 : PERM ? 6 : 4;   // planes of stress-divergence partials that travel through LDS
    constexpr int SW = PERM ? W + 1 : W;      // row stride of a plane (PERM: odd, a column of cells is not one bank)
    constexpr int SP = SW * H;                // plane size
    // LDS (dynamic): s_str[NSTR][SP] | s_tc[4][256] | s_u[NUV] | s_v[NUV] | s_uc[nu][256]
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *s_str = smem;
    double *s_tc = smem + NSTR * SP;
    double *s_u = s_tc + 4 * 256;
    double *s_v = s_u + NUV;
    double *s_uc = s_v + NUV;
    // COOP: per rim T-cell its ten operands (s_rc[k * 64 + g]) and the two partials its own U-cell's thread keeps (s_r04), behind s_uc
    double *s_rc = nullptr, *s_r04 = nullptr;
    __shared__ int s_bad;

    __shared__ int s_chunk[4], s_simd[4], s_cu;
    __shared__ int s_slot[4];                 // RIMU: [0..2] the subcycles whose stress the interior waves have finished

    const int tx = threadIdx.x, ty = threadIdx.y;
    const int t = ty * 64 + tx;
    // launch order = heaviest tiles first (host-sorted by active waves, see resident2_order): the
    // workgroups that end up third on a CU are then the cheap ones (land, partial edge tiles)
    const int tile = R.order ? R.order[blockIdx.x] : (int)blockIdx.x;
    bool no_ucell;
    {
        // A tile that owns no U-cell leaves at once.  The tile grid is uniform over the blocks of a rank (sized for the
        // largest one), so a block that is a row or column shorter than the largest gets a last tile row / column that
        // starts beyond its last U-cell: all such a tile holds is the T-row jhi+1 (or column ihi+1), which the tile below
        // (left of) it computes and stores as well.  It would poll its neighbours' records every subcycle while nobody
        // polls any of its own -- a reader without back-pressure on its producers: they may run two subcycles ahead of
        // it and overwrite a record it has not read, after which it waits for ever (seen as "a wait gave up ... tag
        // seen 0x1002, wanted 0x1000" in the probe of a 3 x 3-block decomposition whose top blocks are one row short;
        // on a single rank the call then fell back to the streaming kernel, across ranks it failed).
        const int pb = A.gx * A.gy;
        const int4 rb = A.blk[tile / pb];
        // (test build, EVP_RES2_HOOK_KEEP_NO_UCELL: keep them, EVP_RES2_HOOK_LAG_NO_UCELL: and let them lag -- to show the hazard, tests/test_gpu_parity.py)
        no_ucell = rb.x + ((tile % pb) % A.gx) * (W - 1) > rb.y || rb.z + ((tile % pb) / A.gx) * (H - 1) > rb.w;
        if (no_ucell && !(RES_DBG(R) & EVP_RES2_HOOK_KEEP_NO_UCELL)) return;
    }
    // what a launch pays beside its subcycles (test build, with the phase stamps; tools/resident_launch_stamps.py): wall-clock stamps
    // of every wave -- workgroup start, after the lock, the lane tables and masks loaded, the state loads issued and landed, the first
    // ring poll matched, the loop's end, the write-back's stores landed
    unsigned long long lst0 = 0, lst1 = 0, lst2 = 0, lst3 = 0, lst4 = 0;
    if (RES_PROF(R)) lst0 = wall_clock64();
    // PERM: which quarter ("chunk") of the tile's permuted cell list this wave takes.  The host packs
    // the ice cells of a tile into its first chunks (a coastal tile then costs one or two waves, not
    // four).  A SIMD issues for one wave at a time and all tiles advance in lock step, so the SIMD with
    // the most ice-holding waves paces the whole grid: the workgroups that share a CU put their active
    // chunks on the CU's least loaded SIMDs (the wave -> SIMD map is the hardware's: read from HW_ID;
    // a small per-CU record under a lock, once per launch).  Speed only: any chunk -> wave map is correct.
    int tq = t;
    int cu_rank = 0;                          // how many workgroups had reached this CU before this one
    // RIMU, full tiles (all four chunks hold ice): such a tile adds one wave to every SIMD's count, so it changes no later
    // comparison and its own map is arbitrary -- it takes the identity map and leaves the per-CU record alone (no CAS, no loads,
    // no stores; the partial tiles' choices are what they were).  The product compiles it in or out (EVP_RES2_NOLOCK_DEFAULT);
    // the test build carries a switch (EVP_RES2_HOOK_NOLOCK, CICE_EVP_HIP_RES_NOLOCK) and keeps the lock for every tile while the
    // stamps are on: the arrival rank feeds them.  profiles/r16_resident_rim_first.txt
#ifdef CICE_EVP_HIP_TESTING
    const bool skip_lock = RIMU && (RES_DBG(R) & EVP_RES2_HOOK_NOLOCK) && !RES_PROF(R);
#else
    constexpr bool skip_lock = RIMU && EVP_RES2_NOLOCK_DEFAULT;
#endif
    bool balance = PERM && R.cuload && !(RES_DBG(R) & EVP_RES2_HOOK_NO_BALANCE);
    if (skip_lock && balance && R.nact[tile] == 4) balance = false;      // (uniform over the workgroup)
    if (balance) {
        const int wave = t >> 6;
        if ((t & 63) == 0) {
            unsigned hw, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            s_simd[wave] = (int)((hw >> 4) & 3u);
            if (wave == 0) s_cu = (int)(((xcc & 7u) << 8) | ((hw >> 8) & 0xffu));   // XCC | SE, SH, CU
        }
        __syncthreads();
        if (t == 0) {
            int *L = R.cuload + 8 * s_cu;         // [0] lock, [1] launch stamp, [2..5] ice-holding waves per SIMD, [6] workgroups so far
            const int nact = R.nact[tile];        // active chunks of this tile: 0 .. nact-1
            int chunk_of[4] = {0, 1, 2, 3};
            unsigned spins = 0;
            bool locked = false;
            // RIMU: the record as ONE 64-bit word (behind the [2048][8] records: launch epoch << 40 | arrivals << 32 | the four SIMD
            // counts, 8 bits each) under a compare-and-swap loop: a load and a swap, one swap more per workgroup of the CU that came
            // in between -- where the lock below takes a swap, the stamp's load, the counts' loads, the stores, their
            // acknowledgement and the unlock, and every later workgroup of the CU waits for all of it.  A word of another launch
            // counts as zeros (epochs start at 1).  The same counts give the same chunk -> wave map.  The product compiles it in or
            // out (EVP_RES2_LOCK_CAS_DEFAULT); the test build carries a switch (EVP_RES2_HOOK_LOCK_CAS, CICE_EVP_HIP_RES_LOCK_CAS).
#ifdef CICE_EVP_HIP_TESTING
            const bool lock_cas = RIMU && (RES_DBG(R) & EVP_RES2_HOOK_LOCK_CAS);
#else
            constexpr bool lock_cas = RIMU && EVP_RES2_LOCK_CAS_DEFAULT;
#endif
            if (lock_cas) {
                unsigned long long *L64 = reinterpret_cast<unsigned long long *>(R.cuload + 2048 * 8) + s_cu;
                const unsigned long long epoch = (unsigned long long)(R.tag_base >> 12);
                unsigned long long seen = __hip_atomic_load(L64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (spins++ < 200000u) {
                    const bool fresh = (seen >> 40) != epoch;
                    int ld[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) ld[q] = fresh ? 0 : (int)((seen >> (8 * q)) & 255u);
                    const int rank = fresh ? 0 : (int)((seen >> 32) & 255u);
                    bool used[4] = {false, false, false, false};
                    for (int ck = 0; ck < 4; ++ck) {      // active chunks first, each to the free wave on the least loaded SIMD
                        int best = -1;
                        for (int w = 0; w < 4; ++w) {
                            if (used[w]) continue;
                            if (best < 0 || ld[s_simd[w] & 3] < ld[s_simd[best] & 3]) best = w;
                        }
                        used[best] = true;
                        chunk_of[best] = ck;
                        if (ck < nact) ld[s_simd[best] & 3] += 1;
                    }
                    const unsigned long long next = (epoch << 40) | ((unsigned long long)((rank + 1) & 255) << 32) |
                                                    ((unsigned long long)(ld[3] & 255) << 24) | ((unsigned long long)(ld[2] & 255) << 16) |
                                                    ((unsigned long long)(ld[1] & 255) << 8) | (unsigned long long)(ld[0] & 255);
                    const unsigned long long was = atomicCAS(L64, seen, next);
                    if (was == seen) { s_simd[0] |= rank << 8; locked = true; break; }
                    seen = was;
                }
                if (!locked) { chunk_of[0] = 0; chunk_of[1] = 1; chunk_of[2] = 2; chunk_of[3] = 3; }      // (gave up: any map is correct)
            } else
            while (spins++ < 200000u) {
                if (atomicCAS(&L[0], 0, 1) == 0) { locked = true; break; }
                __builtin_amdgcn_s_sleep(2);
            }
            if (locked && !lock_cas) {
                int ld[4];
                const int stamp = __hip_atomic_load(&L[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool fresh = stamp != (int)R.tag_base;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    ld[q] = fresh ? 0 : __hip_atomic_load(&L[2 + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int rank = fresh ? 0 : __hip_atomic_load(&L[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_simd[0] |= rank << 8;               // (the arrival rank travels to the other threads with it)
                bool used[4] = {false, false, false, false};
                for (int ck = 0; ck < 4; ++ck) {      // active chunks first, each to the free wave on the least loaded SIMD
                    int best = -1;
                    for (int w = 0; w < 4; ++w) {
                        if (used[w]) continue;
                        if (best < 0 || ld[s_simd[w] & 3] < ld[s_simd[best] & 3]) best = w;
                    }
                    used[best] = true;
                    chunk_of[best] = ck;
                    if (ck < nact) ld[s_simd[best] & 3] += 1;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) __hip_atomic_store(&L[2 + q], ld[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&L[6], rank + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&L[1], (int)R.tag_base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&L[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) s_chunk[w] = chunk_of[w];
        }
        __syncthreads();
        tq = s_chunk[wave] * 64 + (t & 63);
        cu_rank = s_simd[0] >> 8;
        // (tried in round 4 on the two-barrier schedule, no measurable effect on gx1: one s_setprio level per workgroup on
        // all SIMDs of its CU, in either order; s_setprio 3 for the rim wave between its poll and the barrier; rim waves of
        // the workgroups of a CU on different SIMDs; s_sleep 0/3/8 in the poll loop -- all within +-2 %.  There the interior
        // waves sat at B1 while the rim wave worked.  On the rim-wave schedule they step inside its window and priorities do
        // pay: subcycle_rim below)
    }
    // (a launch stamp first waits for the wave's outstanding loads and stores: each span then holds what was issued inside it,
    // and the stamped prologue is the sum of its levels, not their overlap)
#define EVP_LSTAMP(x)                                                       \
    if (RES_PROF(R)) {                                                      \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");         \
        x = wall_clock64();                                                 \
    }
    EVP_LSTAMP(lst1)
    // which T-cell of the tile this thread owns: row-major (lane = column) unless permuted
    const int pos = PERM ? (int)R.perm[tile * 256 + tq] : t;      // == trow*W + tcol
    const int tcol = pos & (W - 1);
    const int trow = pos >> LOGW;
    const int sp = trow * SW + tcol;          // this cell in a plane of s_str
    // PERM: waves below `late_waves` hold the T-cells that read ring velocities and do the ring poll;
    // with exactly one such wave (every 16 x 16 tile: rim <= 60 cells, ring <= 64 entries) the others
    // never wait for it before their stress update ("split")
    const int late_waves = PERM ? (int)R.late_waves[tile] : 4;
    const bool split = PERM && late_waves <= 1 && !(RES_DBG(R) & EVP_RES2_HOOK_NO_RIM_SPLIT);
    if ((RES_DBG(R) & EVP_RES2_HOOK_ABSENT_TILE) && tile == 1 && !R.dry) return;   // test hook: one workgroup "never becomes resident" (after the probes)
    const int per_blk = A.gx * A.gy;
    const int bz = tile / per_blk;                // CICE block of this rank
    const int bx = (tile % per_blk) % A.gx;
    const int by = (tile % per_blk) / A.gx;
    const int4 r = A.blk[bz];
    const int i0 = r.x + bx * (W - 1), j0 = r.z + by * (H - 1);
    const int i = i0 + tcol;
    const int j = j0 + trow;
    const int nx = A.nx, ny = A.ny;
    const int cb = bz * (int)A.plane;             // first cell of the block in every (nx, ny, nblocks) array
    const int c = cb + (j - 1) * nx + (i - 1);
    const int li = (trow + 1) * LW + (tcol + 1);   // this cell in the LDS velocity tile
    // RIMU: the U-cell a thread holds need not sit at its T-cell's position (R.uperm, rim_plan.h; 255: none -- never an owned cell)
    const int upos = RIMU ? (int)R.uperm[tile * 256 + tq] : pos;
    const int ucol = upos & (W - 1), urow = upos >> LOGW;
    const int ui = RIMU ? i0 + ucol : i, uj = RIMU ? j0 + urow : j;
    const int cu = RIMU ? cb + (uj - 1) * nx + (ui - 1) : c;
    const int uli = RIMU ? (urow + 1) * LW + (ucol + 1) : li;
    const int usp = RIMU ? urow * SW + ucol : sp;
    const unsigned flags = A.flags;
    const bool water = !LEAN && !(flags & EVP_F_WATER_IS_OCN);     // (LEAN: launched only with both flags set)
    const bool tbu = !LEAN && !(flags & EVP_F_TBU_ZERO);
    if (COOP) {
        s_rc = s_uc + (8 + (water ? 2 : 0) + (tbu ? 1 : 0)) * 256;
        s_r04 = s_rc + 10 * 64;
    }

    const bool inT = (i <= r.y + 1) && (j <= r.w + 1);
    unsigned m = 0;
    if (inT) m = A.mask[c];
    const bool actT = inT && (m & 1u);
    const bool ownU = (ucol < W - 1) && (urow < H - 1) && (ui <= r.y) && (uj <= r.w);
    unsigned mU = m;
    if (RIMU) mU = ownU ? A.mask[cu] : 0u;
    const bool isU = ownU && (mU & 2u);
    const bool own = (tcol < W - 1 || i == r.y + 1) && (trow < H - 1 || j == r.w + 1);
    // Every U-cell another tile's ring mirrors publishes a record every subcycle, ice or not, and
    // every ring entry that has a producer is polled every subcycle: a tile then cannot run more
    // than one subcycle ahead of ANY tile that still has to read its records (the two-buffer
    // record scheme depends on that; making either side depend on the ice mask would let a tile
    // next to open water run ahead of its reader and overwrite a record that was never read).
    const bool pub = ownU && (R.pubmap[cu] != 0);
    EVP_LSTAMP(lst2)
    const int par0 = R.par0;                      // record buffer of subcycle index 0 in this launch
    // COOP: the first nlate entries of the tile's permuted cell list are its rim T-cells with ice (resident2_order); the
    // thread that holds such a cell leaves its stress update to the quad g = its list index, lanes 4g .. 4g+3 of the workgroup
    const int nlate = COOP ? (int)R.nlate[tile] : 0;
    const bool rim_owner = COOP && tq < nlate;
    const bool actN = actT && !rim_owner;         // this thread updates its own T-cell
    const int g = t >> 2, qc = t & 3;             // quad, corner: 0 NE, 1 NW, 2 SW, 3 SE (the order of the stress arrays)
    const bool quad = COOP && g < nlate;
    int gc = 0;
    unsigned g_vel = 0, g_out = 0;                // packed LDS indices: the three velocity cells (10 bits each), the two outputs (16 bits each)
    bool gown = false;
    double sr0 = 0.0, sr1 = 0.0, sr2 = 0.0;       // stressp_q, stressm_q, stress12_q of the quad's cell
    if (quad) {
        const int gpos = (int)R.perm[tile * 256 + g];
        const int gcol = gpos & (W - 1), grow = gpos >> LOGW;
        const int gi = i0 + gcol, gj = j0 + grow;
        gc = cb + (gj - 1) * nx + (gi - 1);
        gown = (gcol < W - 1 || gi == r.y + 1) && (grow < H - 1 || gj == r.w + 1);
        const int gli = (grow + 1) * LW + (gcol + 1);
        const int ij = gli, im = gli - 1, jm = gli - LW, mm = gli - LW - 1;
        // the corner's operands: first / second velocity of the u-pair, second of the v-pair (the first is the same cell)
        const int g_oa = qc == 0 ? ij : qc == 1 ? im : qc == 2 ? mm : jm;
        const int g_ob = qc == 0 ? im : qc == 1 ? ij : qc == 2 ? jm : mm;
        const int g_od = qc == 0 ? jm : qc == 1 ? mm : qc == 2 ? im : ij;
        g_vel = (unsigned)g_oa | ((unsigned)g_ob << 10) | ((unsigned)g_od << 20);
        // where the lane's two partials go: NE str(1), str(5) -> the cell's own thread (s_r04); NW str(2), str(7) -> planes 4, 5;
        // SW str(4), str(8) -> planes 2, 3; SE str(3), str(6) -> planes 0, 1
        const int gsp = grow * SW + gcol;
        const int off04 = (int)(s_r04 - s_str);   // (indices relative to s_str: the NE lane's two go to s_r04)
        const int g_ox = qc == 0 ? off04 + g : (qc == 1 ? 4 : qc == 2 ? 2 : 0) * SP + gsp;
        const int g_oy = qc == 0 ? off04 + 64 + g : (qc == 1 ? 5 : qc == 2 ? 3 : 1) * SP + gsp;
        g_out = (unsigned)g_ox | ((unsigned)g_oy << 16);
        sr0 = R.tab[R.cur0 * 12 + qc][gc];
        sr1 = R.tab[R.cur0 * 12 + 4 + qc][gc];
        sr2 = R.tab[R.cur0 * 12 + 8 + qc][gc];
        if (qc == 0) {
            typename MM::SI b;
            b.dxT = A.dxT[gc]; b.dyT = A.dyT[gc];
            b.strength = A.strength[gc];
            if ((flags & EVP_F_METRICS) && !(flags & EVP_F_DXHY_ARRAY)) {
                MM::metrics(A.HTE[gc], A.HTE[gc - 1], A.HTN[gc], A.HTN[gc - nx], A.deltaminEVP, b);
            } else {
                b.dxhy = A.dxhy[gc]; b.dyhx = A.dyhx[gc];
                b.cxp = A.cxp[gc]; b.cyp = A.cyp[gc]; b.cxm = A.cxm[gc]; b.cym = A.cym[gc];
                b.DminTarea = A.DminTarea[gc];
            }
            s_rc[0 * 64 + g] = b.strength; s_rc[1 * 64 + g] = b.DminTarea;
            s_rc[2 * 64 + g] = b.dxT; s_rc[3 * 64 + g] = b.dyT;
            s_rc[4 * 64 + g] = b.cxp; s_rc[5 * 64 + g] = b.cyp; s_rc[6 * 64 + g] = b.cxm; s_rc[7 * 64 + g] = b.cym;
            s_rc[8 * 64 + g] = b.dxhy; s_rc[9 * 64 + g] = b.dyhx;
        }
    }

    // ---- state that stays on the CU for the whole call -------------------------------------
    typename MM::SI a;
    double s[12];
    POL pol;
    bool percall_out = false;
    if (actN) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = R.tab[R.cur0 * 12 + k][c];
        a.dxT = A.dxT[c]; a.dyT = A.dyT[c];
        a.strength = A.strength[c];
        if ((flags & EVP_F_METRICS) && !(flags & EVP_F_DXHY_ARRAY)) {
            MM::metrics(A.HTE[c], A.HTE[c - 1], A.HTN[c], A.HTN[c - nx], A.deltaminEVP, a);
        } else {
            a.dxhy = A.dxhy[c]; a.dyhx = A.dyhx[c];
            a.cxp = A.cxp[c]; a.cyp = A.cyp[c]; a.cxm = A.cxm[c]; a.cym = A.cym[c];
            a.DminTarea = A.DminTarea[c];
        }
        s_tc[0 * 256 + t] = a.strength;
        s_tc[1 * 256 + t] = a.DminTarea;
        s_tc[2 * 256 + t] = a.dxhy;
        s_tc[3 * 256 + t] = a.dyhx;
        if constexpr (POL::ranged) percall_out = POL::percall_outside(a.strength, a.DminTarea);
    }
    if constexpr (POL::ranged) {
        pol.cbad = __builtin_amdgcn_ballot_w64(percall_out);
        pol.off = (RES_DBG(R) & EVP_RES2_HOOK_NO_RANGE) != 0;
#ifdef CICE_EVP_HIP_TESTING
        pol.nosplit = !(RES_DBG(R) & EVP_RES2_HOOK_SPLITDIV);
#endif
    }
    const POLE &pole = pol;
    if (isU) {
        s_uc[0 * 256 + t] = A.vrelfac[cu];
        s_uc[1 * 256 + t] = A.uocn[cu];
        s_uc[2 * 256 + t] = A.vocn[cu];
        s_uc[3 * 256 + t] = A.forcex[cu];
        s_uc[4 * 256 + t] = A.forcey[cu];
        s_uc[5 * 256 + t] = A.umassdti[cu];
        s_uc[6 * 256 + t] = A.fm[cu];
        s_uc[7 * 256 + t] = A.uarear[cu];
        int row = 8;
        if (water) { s_uc[row * 256 + t] = A.waterx[cu]; s_uc[(row + 1) * 256 + t] = A.watery[cu]; row += 2; }
        if (tbu) s_uc[row * 256 + t] = A.TbU[cu];
    }
    // the velocity tile incl. its ring starts from the input arrays (ghost cells are valid on entry)
    {
        const double *u0 = R.u[R.cur0], *v0 = R.v[R.cur0];
        for (int q = t; q < (H + 1) * LW; q += 256) {
            const int pr = q / LW - 1, pc = q % LW - 1;
            const int gi = i0 + pc, gj = j0 + pr;
            double uu = 0.0, vv = 0.0;
            if (gi >= 1 && gi <= nx && gj >= 1 && gj <= ny) {
                const int cp = cb + (gj - 1) * nx + (gi - 1);
                uu = u0[cp]; vv = v0[cp];
            }
            s_u[q] = uu; s_v[q] = vv;
        }
    }
    // ghost images of this U-cell (cyclic wrap), looked up once: at most three (corner cell)
    int img0 = -1, img1 = -1, img2 = -1;
    // tripole seam (row jhi lies on the fold): this thread's U-cell takes part in the pair average
    // after every momentum step, ice or not (ice_boundary.F90:1630-1649) -- role 1/2: low/high index
    // of a pair, 3: pole point; partner = the other cell of the pair
    int seam_role = 0, seam_partner = -1;
    if (!LEAN && R.seam && ownU && j == r.w) {
        const int sv = R.seam[bz * nx + i - 1];
        seam_role = sv & 3;
        seam_partner = sv >> 2;
    }
    const bool isSeam = seam_role != 0;
    if (!LEAN && R.img3) {
        // tripole: ghost images are not confined to the block edge (ghost row NY+1 mirrors row NY-1):
        // per-cell table, at most three images
        if (ownU) { img0 = R.img3[3 * c]; img1 = R.img3[3 * c + 1]; img2 = R.img3[3 * c + 2]; }
    } else
    if (ownU && (flags & EVP_F_PUSH) && (ui == r.x || ui == r.y || uj == r.z || uj == r.w)) {
        const int slots[4] = {(ui == r.x) ? (uj - r.z) : -1, (ui == r.y) ? A.push_nj + (uj - r.z) : -1,
                              (uj == r.z) ? 2 * A.push_nj + (ui - r.x) : -1,
                              (uj == r.w) ? 2 * A.push_nj + A.push_ni + (ui - r.x) : -1};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (slots[e] < 0) continue;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const int v = A.push[slots[e] * 2 + w];
                if (v < 0) continue;
                if (img0 < 0) img0 = v;
                else if (img1 < 0) img1 = v;
                else img2 = v;
            }
        }
    }
    // images of this U-cell on other ranks: record address (parity 0) in the peer's buffer
    char *rp0 = nullptr, *rp1 = nullptr, *rp2 = nullptr;
    size_t rs0 = 0, rs1 = 0, rs2 = 0;
    double rg0 = 1.0, rg1 = 1.0, rg2 = 1.0;       // an image across the tripole fold takes the negative
    // fold row split over ranks: where this seam cell's RAW record goes on other ranks
    char *rq0 = nullptr, *rq1 = nullptr, *rq2 = nullptr;
    size_t rqs0 = 0, rqs1 = 0, rqs2 = 0;
    if (REMOTE) {
        if (ownU) {
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int2 v = R.rimg[3 * (size_t)c + e];      // per-cell table: {peer index (| 256: negative), ghost cell at that peer}
                if (v.x < 0) continue;
                const int pe = v.x & 255;
                char *ptr = (char *)R.peer_rec[pe] + 32 * (size_t)v.y;
                const size_t st = R.peer_rstride[pe];
                const double sg = (v.x & 256) ? -1.0 : 1.0;
                if (!rp0) { rp0 = ptr; rs0 = st; rg0 = sg; }
                else if (!rp1) { rp1 = ptr; rs1 = st; rg1 = sg; }
                else { rp2 = ptr; rs2 = st; rg2 = sg; }
            }
            if (R.rraw && isSeam) {
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int2 v = R.rraw[3 * (size_t)c + e];
                    if (v.x < 0) continue;
                    char *ptr = (char *)R.peer_raw[v.x] + 32 * (size_t)v.y;
                    const size_t st = R.peer_raw_stride[v.x];
                    if (!rq0) { rq0 = ptr; rqs0 = st; }
                    else if (!rq1) { rq1 = ptr; rqs1 = st; }
                    else { rq2 = ptr; rqs2 = st; }
                }
            }
        }
    }
    // the partner of a seam pair on another rank: its raw record arrives in THIS rank's rec_raw buffer at a staging slot
    const bool seam_remote = REMOTE && isSeam && seam_role != 3 && seam_partner >= (int)(A.plane * (size_t)R.nblocks);
    const bool rpub = REMOTE && rp0 != nullptr;    // publishes every subcycle, ice or not
    // my ring entry: which cell of the LDS ring do I refresh, from which record
    int ring_cp = -1, ring_li = 0;
    bool ring_remote = false;
    if (tq < R.ring_cnt[tile]) {     // (PERM: ring entries and the T-cells that read them share the wave that took chunk 0)
        const int4 e = R.ring[tile * EVP_RES2_RING + tq];   // x: cell whose record is polled, y: LDS index, z: producing U-cell
        // has a producer on this GPU: refreshed every subcycle -- unless the producer's tile holds no ice and does not run
        // (EvpResident2::live): its cells keep the values the velocity tile was filled with above
        if (e.z >= 0 && (!R.live || R.live[R.celltile[e.z]])) { ring_cp = e.x; ring_li = e.y; }
        if (REMOTE && e.z == -2) { ring_cp = e.x; ring_li = e.y; ring_remote = true; }   // produced on another rank
    }
    // first wait that gives up records where and on what: err[0] kind (1 ring of this GPU, 2 ring of
    // another rank, 3 fold-row partner, 4 final ghosts), [1] tile, [2] subcycle, [3] cell, [4] tag seen, [5] tag wanted
    auto give_up_note = [&](int kind, int k, int cell, unsigned seen, unsigned wanted) {
        if (atomicCAS(R.err, 0, kind) == 0) {
            R.err[1] = tile; R.err[2] = k; R.err[3] = cell; R.err[4] = (int)seen; R.err[5] = (int)wanted;
        }
    };
    auto publish_remote = [&](int par, double uu, double vv, unsigned tag) {
        st_rec2_sys(rp0 + (size_t)par * rs0, pack_rec(rg0 * uu, tag), pack_rec(rg0 * vv, tag));
        if (rp1) st_rec2_sys(rp1 + (size_t)par * rs1, pack_rec(rg1 * uu, tag), pack_rec(rg1 * vv, tag));
        if (rp2) st_rec2_sys(rp2 + (size_t)par * rs2, pack_rec(rg2 * uu, tag), pack_rec(rg2 * vv, tag));
    };
    // one poll of a record written by another rank: bounded by wall-clock time (ranks reach
    // evp() at different moments), not by a spin count
    auto poll_remote = [&](const v4u *rec, unsigned want, v4u &ra, v4u &rb, int kind = 2, int cell = -1) -> bool {
        const unsigned long long t0 = wall_clock64();
        unsigned spins = 0;
        for (;;) {
            ld_rec2_sys(rec, ra, rb);
            if (ra.x == want && ra.w == want && rb.x == want && rb.w == want) return true;
            if ((++spins & 255u) == 0 &&
                (wall_clock64() - t0 > R.timeout_ticks ||
                 __hip_atomic_load(R.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                give_up_note(kind, (int)(want - R.tag_base), cell >= 0 ? cell : ring_cp, ra.x, want);
                return false;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    };
    if (t == 0) s_bad = 0;
    if (RIMU) {
        // a plane entry is written by the thread of an ice T-cell only: the others stay zero for the whole call
        for (int q = t; q < NSTR * SP; q += 256) s_str[q] = 0.0;
        if (t < 4) s_slot[t] = 0;
    }
    EVP_LSTAMP(lst3)
    __syncthreads();

    // bound of a wait on a record of this GPU: spin count (workgroups not co-resident -> fail fast) on
    // a rank without remote neighbours, wall-clock time otherwise
    unsigned long long t_wait0 = 0;
    auto gave_up = [&](unsigned spins, unsigned long long t0) -> bool {
        if (REMOTE) {
            if ((spins & 255u) != 0) return false;
            return wall_clock64() - t0 > R.timeout_ticks ||
                   __hip_atomic_load(R.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        }
        return spins > R.spin_limit ||
               ((spins & 255u) == 0 && __hip_atomic_load(R.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
    };
    double u_own = 0.0, v_own = 0.0;
    if (ownU) { u_own = s_u[uli]; v_own = s_v[uli]; }
    // initial records (subcycle tag 0) so that the neighbours' first ring refresh finds them
    {
        const unsigned tag = R.tag_base;
        v4u *r0 = (v4u *)R.rec[par0 & 1];
        if (rpub) publish_remote(par0 & 1, u_own, v_own, tag);
        if (pub) st_rec2(r0 + 2 * (size_t)cu, pack_rec(u_own, tag), pack_rec(v_own, tag));
        if (ownU) {
            if (img0 >= 0) { const double sg = (img0 & 1) ? -1.0 : 1.0; st_rec2(r0 + 2 * (size_t)(img0 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
            if (img1 >= 0) { const double sg = (img1 & 1) ? -1.0 : 1.0; st_rec2(r0 + 2 * (size_t)(img1 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
            if (img2 >= 0) { const double sg = (img2 & 1) ? -1.0 : 1.0; st_rec2(r0 + 2 * (size_t)(img2 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
        }
    }

    // ---- the subcycle loop (ice_dyn_evp.F90:859-913) ------------------------------------------
    // optional phase stamps of every wave (CICE_EVP_HIP_RES_PROF=1, tools/resident_phases.py): shader cycles
    // spent in [ring poll | stress | wait at the barrier before the momentum step | momentum step, seam,
    // publish | wait at the barrier that ends the subcycle]
    const bool prof = RES_PROF(R);
    unsigned long long pc0 = 0, pacc0 = 0, pacc1 = 0, pacc2 = 0, pacc3 = 0, pacc4 = 0;
    if (prof) pc0 = __builtin_readcyclecounter();
#define EVP_STAMP(acc)                                                  \
    if (prof) {                                                         \
        const unsigned long long now_ = __builtin_readcyclecounter();   \
        acc += now_ - pc0;                                              \
        pc0 = now_;                                                     \
    }
    // Tried in round 4 on the two-barrier schedule (subcycle below), measured on gx1 (tools/resident_phases.py; DESIGN.md section
    // 4), none moved the subcycle by more than 2 %: s_setprio 3 for the rim wave / 0 for interior stress / 2 for every wave's
    // momentum step (on the rim-wave schedule priorities take 5-7 % off the step: subcycle_rim); the ring records of the
    // next subcycle requested before the momentum step (the hand-off is on a dependency CYCLE between neighbours, not on one
    // tile's critical path: nothing is there earlier); fine-grained / uncached memory for the record buffers; no s_sleep.
    // Two polls in flight per lane (a second poll a few hundred cycles behind the first, each re-issued once looked at; one
    // asm block on fixed registers, compares included -- the compiler copies a poll's registers at a loop merge while the
    // load is in flight, in every form it was given): bit-identical, and SLOWER -- poll phase 4476 -> 5131 cycles, 4.69 ->
    // 4.90 us per subcycle (gpurun_out/r4i): twice the poll traffic costs more than the earlier sighting saves.
    // LEAN: record addresses are a scalar base (the buffer of the subcycle's parity) plus a 32-bit lane offset fixed for the call
    const unsigned ring_off = 32u * (unsigned)(ring_cp >= 0 ? ring_cp : 0);
    const unsigned own_off = 32u * (unsigned)cu;
    const unsigned img_off0 = 32u * (unsigned)(img0 >> 1), img_off1 = 32u * (unsigned)(img1 >> 1), img_off2 = 32u * (unsigned)(img2 >> 1);
    const double img_sg0 = (img0 & 1) ? -1.0 : 1.0, img_sg1 = (img1 & 1) ? -1.0 : 1.0, img_sg2 = (img2 & 1) ? -1.0 : 1.0;
    // one subcycle: reads the records of buffer rd, writes those of buffer wr; false: a wait gave up, the workgroup leaves
    auto subcycle = [&](const int k, const v4u *rd, v4u *wr) -> bool {
        const unsigned want = R.tag_base + (unsigned)k;       // tag of the velocities subcycle k reads

        if (((RES_DBG(R) & EVP_RES2_HOOK_LAG) && (tile & 3) == 1) || ((RES_DBG(R) & EVP_RES2_HOOK_LAG_NO_UCELL) && no_ucell)) {      // robustness test: every fourth tile lags by ~10 us per subcycle
            const unsigned long long t0 = wall_clock64();
            while (wall_clock64() - t0 < 1000ull) __builtin_amdgcn_s_sleep(8);
        }
        // refresh the ring of the velocity tile from the neighbours' records (split: only wave 0 holds
        // ring entries and T-cells that read them; nobody else waits here)
        if (REMOTE && ring_remote) {
            v4u ra, rb;
            if (!poll_remote(rd + 2 * (size_t)ring_cp, want, ra, rb)) s_bad = 1;
            s_u[ring_li] = unpack_rec(ra);
            s_v[ring_li] = unpack_rec(rb);
        } else if (ring_cp >= 0 && !(RES_DBG(R) & EVP_RES2_HOOK_NO_RING_LOADS)) {
            v4u ra, rb;
            unsigned spins = 0;
            if (REMOTE) t_wait0 = wall_clock64();
            for (;;) {
                if (LEAN) ld_rec2_s(rd, ring_off, ra, rb);
                else ld_rec2(rd + 2 * (size_t)ring_cp, ra, rb);
                if ((ra.x == want && ra.w == want && rb.x == want && rb.w == want) || (RES_DBG(R) & EVP_RES2_HOOK_NO_TAG_CHECK)) break;
                // a local neighbour may itself be waiting for another rank: with remote neighbours
                // every wait is bounded by wall-clock time, not by a spin count
                if (gave_up(++spins, t_wait0)) {
                    give_up_note(1, k, ring_cp, ra.x, want);
                    s_bad = 1;
                    break;
                }
                if (RES_DBG(R) & EVP_RES2_HOOK_LONG_SLEEP) __builtin_amdgcn_s_sleep(8); else __builtin_amdgcn_s_sleep(1);
            }
            s_u[ring_li] = unpack_rec(ra);
            s_v[ring_li] = unpack_rec(rb);
        }
        if (!split) {
            __syncthreads();
            if (s_bad) return false;   // uniform: every thread of the workgroup leaves together
        } else {
            // ring cells are written and read by wave 0 only: LDS operations of one wave complete in order
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        EVP_STAMP(pacc0)
        if (prof && k == 0) lst4 = wall_clock64();

        double str[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) str[e] = 0.0;
        if (actN) {
            a.u_ij = s_u[li]; a.v_ij = s_v[li];
            a.u_im = s_u[li - 1]; a.v_im = s_v[li - 1];
            a.u_jm = s_u[li - LW]; a.v_jm = s_v[li - LW];
            a.u_mm = s_u[li - LW - 1]; a.v_mm = s_v[li - LW - 1];
            a.strength = s_tc[0 * 256 + t]; a.DminTarea = s_tc[1 * 256 + t];
            a.dxhy = s_tc[2 * 256 + t]; a.dyhx = s_tc[3 * 256 + t];
            MM::template stress<CAP, POLE>(A.p, a, s, str, pole);
        }
        EVP_STAMP(pacc1)
        double sx1, sy2;
        if (PERM) {      // by cell position: the U-cell's thread need not sit next to its T neighbours
            if (!rim_owner) {      // (COOP: a rim cell's partials come from its quad)
                s_str[0 * SP + sp] = str[2];
                s_str[1 * SP + sp] = str[5];
                s_str[2 * SP + sp] = str[3];
                s_str[3 * SP + sp] = str[7];
                s_str[4 * SP + sp] = str[1];
                s_str[5 * SP + sp] = str[6];
            }
            __syncthreads();
            if (split && s_bad) return false;   // set by wave 0 before the barrier
            if (COOP) {
                EVP_STAMP(pacc2)      // (stamps: the wait at this barrier counts as "wait B1", the quads' work as "stress")
                // the ring is in LDS for everybody now: the rim T-cells, one corner per lane, all four waves
                if (quad) {
                    typename MM::CI cn;
                    double KX, K12X, KYP, K12Y;
                    MM::corner_operands(qc, s_rc[2 * 64 + g], s_rc[3 * 64 + g], s_rc[4 * 64 + g], s_rc[5 * 64 + g], s_rc[6 * 64 + g],
                                        s_rc[7 * 64 + g], cn, KX, K12X, KYP, K12Y);
                    unsigned pv = g_vel, po = g_out;
                    asm volatile("" : "+v"(pv), "+v"(po));      // (unpacked here, every subcycle: not five registers for the whole call)
                    const int g_oa = (int)(pv & 1023u), g_ob = (int)((pv >> 10) & 1023u), g_od = (int)(pv >> 20);
                    cn.ua = s_u[g_oa]; cn.va = s_v[g_oa];
                    cn.ub = s_u[g_ob]; cn.vb = s_v[g_ob];
                    cn.ud = s_u[g_od]; cn.vd = s_v[g_od];
                    cn.strength = s_rc[0 * 64 + g]; cn.DminTarea = s_rc[1 * 64 + g];
                    MM::template corner<CAP>(A.p, cn, sr0, sr1, sr2);
                    double X, Y;
                    MM::partials(sr0, quad_perm<QP_X1>(sr0), quad_perm<QP_X2>(sr0), quad_perm<QP_X3>(sr0),
                                 sr1, quad_perm<QP_X1>(sr1), quad_perm<QP_X2>(sr1), quad_perm<QP_X3>(sr1),
                                 sr2, quad_perm<QP_X1>(sr2), quad_perm<QP_X2>(sr2), quad_perm<QP_X3>(sr2),
                                 KX, K12X, KYP, K12Y, s_rc[8 * 64 + g], s_rc[9 * 64 + g], X, Y);
                    s_str[po & 0xffffu] = X;
                    s_str[po >> 16] = Y;
                }
                EVP_STAMP(pacc1)
                __syncthreads();
                if (rim_owner) { str[0] = s_r04[tq]; str[4] = s_r04[64 + tq]; }
            }
            sx1 = s_str[4 * SP + sp + 1];   // (sp + 1 < SP also for the last cell of the last row: SW = W + 1)
            sy2 = s_str[5 * SP + sp + 1];
        } else {
            s_str[0 * SP + sp] = str[2];
            s_str[1 * SP + sp] = str[5];
            s_str[2 * SP + sp] = str[3];
            s_str[3 * SP + sp] = str[7];
            sx1 = __shfl_down(str[1], 1);
            sy2 = __shfl_down(str[6], 1);
            __syncthreads();
        }
        EVP_STAMP(pacc2)

        if (isU) {
            typename MM::UI q;
            typename MM::UO o;
            q.uold = u_own; q.vold = v_own;
            q.vrelfac = s_uc[0 * 256 + t]; q.uocn = s_uc[1 * 256 + t]; q.vocn = s_uc[2 * 256 + t];
            q.forcex = s_uc[3 * 256 + t]; q.forcey = s_uc[4 * 256 + t]; q.Umassdti = s_uc[5 * 256 + t];
            q.fm = s_uc[6 * 256 + t]; q.uarear = s_uc[7 * 256 + t];
            int row = 8;
            if (water) { q.waterx = s_uc[row * 256 + t]; q.watery = s_uc[(row + 1) * 256 + t]; row += 2; }
            else { q.waterx = q.uocn; q.watery = q.vocn; }
            q.TbU = tbu ? s_uc[row * 256 + t] : 0.0;
            q.uvel_init = !LEAN && A.p.revp != 0.0 ? A.uvel_init[c] : 0.0;
            q.vvel_init = !LEAN && A.p.revp != 0.0 ? A.vvel_init[c] : 0.0;
            q.sx0 = str[0]; q.sx1 = sx1;
            q.sx2 = s_str[0 * SP + sp + SW]; q.sx3 = s_str[2 * SP + sp + SW + 1];
            q.sy0 = str[4]; q.sy1 = s_str[1 * SP + sp + SW];
            q.sy2 = sy2; q.sy3 = s_str[3 * SP + sp + SW + 1];
            if (tbu) MM::template stepu<CAP, true, POLE>(A.p, q, o, pole);
            else MM::template stepu<CAP, false, POLE>(A.p, q, o, pole);
            u_own = o.u; v_own = o.v;
            if (k == R.ndte - 1 && !R.dry) {
                R.tab[24][c] = o.strintx; R.tab[25][c] = o.strinty;
                R.tab[26][c] = o.taubx; R.tab[27][c] = o.tauby;
            }
        }
        // T-fold: a top-row cell waits for the record of the cell it is the image of -- which may sit in the SAME wave (next to the
        // pole columns) and publishes further down: every cell that is not such an image publishes first
        bool published = false;
        if (!LEAN && R.tfold && !isSeam) {
            if (ownU) {
                const unsigned tag = want + 1u;
                if (pub) st_rec2(wr + 2 * (size_t)c, pack_rec(u_own, tag), pack_rec(v_own, tag));
                if (img0 >= 0) { const double sg = (img0 & 1) ? -1.0 : 1.0; st_rec2(wr + 2 * (size_t)(img0 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
                if (img1 >= 0) { const double sg = (img1 & 1) ? -1.0 : 1.0; st_rec2(wr + 2 * (size_t)(img1 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
                if (img2 >= 0) { const double sg = (img2 & 1) ? -1.0 : 1.0; st_rec2(wr + 2 * (size_t)(img2 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
            }
            if (rpub) publish_remote(((k + par0) & 1) ^ 1, u_own, v_own, want + 1u);
            published = true;
        }
        if (isSeam) {
            // what the halo update does to the fold row after every subcycle: pair (a, b) <- (xavg, -xavg),
            // xavg = 0.5*(x_a + isign*x_b), isign = -1; pole points change sign.  The partner's value of
            // THIS subcycle travels as a tagged record of its own (rec_raw), like any other hand-off.
            const double isign = -1.0;
            const unsigned tag = want + 1u;
            if (R.tfold) {
                // T-fold: the top physical row is the image of row NY-1 (a(i, NY) <- -a(NX-i+1, NY-1), nothing averaged).  The cell's own
                // momentum step above has left its strintx / taubx; its velocity is the source cell's FINAL value of this subcycle,
                // which that cell publishes like any velocity another tile mirrors
                v4u ra, rb;
                unsigned spins = 0;
                if (REMOTE) t_wait0 = wall_clock64();
                for (;;) {
                    ld_rec2(wr + 2 * (size_t)seam_partner, ra, rb);
                    if (ra.x == tag && ra.w == tag && rb.x == tag && rb.w == tag) {
                        u_own = isign * unpack_rec(ra); v_own = isign * unpack_rec(rb);
                        break;
                    }
                    if (gave_up(++spins, t_wait0)) {
                        give_up_note(3, k, seam_partner, ra.x, tag);
                        s_bad = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            } else if (seam_role == 3) {
                u_own = isign * u_own; v_own = isign * v_own;
            } else {
                v4u *rw = (v4u *)R.rec_raw[((k + par0) & 1) ^ 1];
                st_rec2(rw + 2 * (size_t)c, pack_rec(u_own, tag), pack_rec(v_own, tag));
                if (REMOTE && rq0) {       // ... and into the rec_raw buffers of the ranks that hold the partner (or an image)
                    const int parw = ((k + par0) & 1) ^ 1;
                    const v4u a = pack_rec(u_own, tag), b = pack_rec(v_own, tag);
                    st_rec2_sys(rq0 + (size_t)parw * rqs0, a, b);
                    if (rq1) st_rec2_sys(rq1 + (size_t)parw * rqs1, a, b);
                    if (rq2) st_rec2_sys(rq2 + (size_t)parw * rqs2, a, b);
                }
                v4u ra, rb;
                unsigned spins = 0;
                bool ok = true;
                if (REMOTE) t_wait0 = wall_clock64();
                if (seam_remote) {
                    ok = poll_remote(rw + 2 * (size_t)seam_partner, tag, ra, rb, 3, seam_partner);
                    if (!ok) s_bad = 1;
                } else
                for (;;) {
                    ld_rec2(rw + 2 * (size_t)seam_partner, ra, rb);
                    if (ra.x == tag && ra.w == tag && rb.x == tag && rb.w == tag) break;
                    if (gave_up(++spins, t_wait0)) {
                        give_up_note(3, k, seam_partner, ra.x, tag);
                        ok = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (ok) {
                    const double pu = unpack_rec(ra), pv = unpack_rec(rb);
                    if (seam_role == 1) {
                        u_own = 0.5 * (u_own + isign * pu);
                        v_own = 0.5 * (v_own + isign * pv);
                    } else {
                        u_own = isign * (0.5 * (pu + isign * u_own));
                        v_own = isign * (0.5 * (pv + isign * v_own));
                    }
                }
            }
        }
        if (isU || isSeam) { s_u[li] = u_own; s_v[li] = v_own; }   // read by the next stress phase (after the ring barrier)
        if (LEAN && ownU) {
            const unsigned tag = want + 1u;
            if (pub) st_rec2_s(wr, own_off, pack_rec(u_own, tag), pack_rec(v_own, tag));
            if (img0 >= 0) st_rec2_s(wr, img_off0, pack_rec(img_sg0 * u_own, tag), pack_rec(img_sg0 * v_own, tag));
            if (img1 >= 0) st_rec2_s(wr, img_off1, pack_rec(img_sg1 * u_own, tag), pack_rec(img_sg1 * v_own, tag));
            if (img2 >= 0) st_rec2_s(wr, img_off2, pack_rec(img_sg2 * u_own, tag), pack_rec(img_sg2 * v_own, tag));
        } else if (ownU && !published) {
            const unsigned tag = want + 1u;
            if (pub) st_rec2(wr + 2 * (size_t)c, pack_rec(u_own, tag), pack_rec(v_own, tag));
            if (img0 >= 0) { const double sg = (img0 & 1) ? -1.0 : 1.0; st_rec2(wr + 2 * (size_t)(img0 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
            if (img1 >= 0) { const double sg = (img1 & 1) ? -1.0 : 1.0; st_rec2(wr + 2 * (size_t)(img1 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
            if (img2 >= 0) { const double sg = (img2 & 1) ? -1.0 : 1.0; st_rec2(wr + 2 * (size_t)(img2 >> 1), pack_rec(sg * u_own, tag), pack_rec(sg * v_own, tag)); }
        }
        if (rpub && !published) publish_remote(((k + par0) & 1) ^ 1, u_own, v_own, want + 1u);
        // no publish step: the records carry their own tags
        EVP_STAMP(pacc3)
        if (split) __syncthreads();   // the tile's own new velocities are in LDS before anybody's next stress update
        EVP_STAMP(pacc4)
        return true;
    };
    // RIMU: the same subcycle on the schedule argued in the header.  rimw: this wave took chunk 0 (ring poll, L_T, L_U)
    const bool rimw = RIMU && __builtin_amdgcn_readfirstlane(tq >> 6) == 0;      // (wave-uniform, and known to be)
    typename MM::UP upre;                         // rim wave: the part of the next momentum step that reads no stress partial
    auto ucell_operands = [&](typename MM::UI &q) {
        q.uold = u_own; q.vold = v_own;
        q.vrelfac = s_uc[0 * 256 + t]; q.uocn = s_uc[1 * 256 + t]; q.vocn = s_uc[2 * 256 + t];
        q.forcex = s_uc[3 * 256 + t]; q.forcey = s_uc[4 * 256 + t]; q.Umassdti = s_uc[5 * 256 + t];
        q.fm = s_uc[6 * 256 + t]; q.uarear = s_uc[7 * 256 + t];
        q.waterx = q.uocn; q.watery = q.vocn;     // (LEAN: water == ocean current, TbU == 0, revp == 0)
        q.TbU = 0.0; q.uvel_init = 0.0; q.vvel_init = 0.0;
    };
    if constexpr (RIMU) if (rimw && isU) {
        typename MM::UI q;
        ucell_operands(q);
        MM::template stepu_pre<CAP, false, POL>(A.p, q, upre, pol);
    }
    // Issue priorities (s_setprio) on this schedule, where the interior waves' momentum step runs inside the rim wave's window
    // and other tiles' waves issue between the rim wave's instructions (profiles/r16_resident_rim_first.txt).  Forms:
    //   1  the rim wave at level 3 from the moment every lane's poll has matched until its records are stored, 0 otherwise;
    //   2  as 1, and the interior waves at level 1 during their stress update;
    //   3  as 1, and the interior waves at level 1 throughout their arithmetic.
    // Every spin (ring poll, slot spin), the barrier and the rim wave's first part after the barrier run at level 0: a spinning
    // wave never outranks a wave that has work.  No bit depends on it.  The product compiles one form in (EVP_RES2_PRIO_DEFAULT,
    // 0: none); the test build carries a switch (EVP_RES2_HOOK_PRIO_MASK: the form; CICE_EVP_HIP_RES_PRIO).
#ifdef CICE_EVP_HIP_TESTING
    const int prio_form = RIMU ? (RES_DBG(R) & EVP_RES2_HOOK_PRIO_MASK) >> EVP_RES2_HOOK_PRIO_SHIFT : 0;
#else
    constexpr int prio_form = RIMU ? EVP_RES2_PRIO_DEFAULT : 0;
#endif
    const bool prio_rim = prio_form != 0 && rimw;                 // (wave-uniform, like rimw)
    const bool prio_in_stress = prio_form >= 2 && !rimw;
    const bool prio_in_step = prio_form == 3 && !rimw;
    auto subcycle_rim = [&](const int k, const v4u *rd, v4u *wr) -> bool {
        const unsigned want = R.tag_base + (unsigned)k;       // tag of the velocities subcycle k reads
        const int done = k + 1;                               // what an interior wave's slot says once its stress of subcycle k is in the planes
        if ((RES_DBG(R) & EVP_RES2_HOOK_LAG) && (tile & 3) == 1) {            // robustness test: every fourth tile lags by ~10 us per subcycle
            const unsigned long long t0 = wall_clock64();
            while (wall_clock64() - t0 < 1000ull) __builtin_amdgcn_s_sleep(8);
        }
        int bad = 0;
        if (rimw) {
            bool gave = false;
            if (ring_cp >= 0 && !(RES_DBG(R) & EVP_RES2_HOOK_NO_RING_LOADS)) {
                v4u ra, rb;
                unsigned spins = 0;
                for (;;) {
                    ld_rec2_s(rd, ring_off, ra, rb);
                    if ((ra.x == want && ra.w == want && rb.x == want && rb.w == want) || (RES_DBG(R) & EVP_RES2_HOOK_NO_TAG_CHECK)) break;
                    if (gave_up(++spins, t_wait0)) {
                        give_up_note(1, k, ring_cp, ra.x, want);
                        __hip_atomic_store(&s_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        gave = true;
                        break;
                    }
                    if (RES_DBG(R) & EVP_RES2_HOOK_LONG_SLEEP) __builtin_amdgcn_s_sleep(8); else __builtin_amdgcn_s_sleep(1);
                }
                s_u[ring_li] = unpack_rec(ra);
                s_v[ring_li] = unpack_rec(rb);
            }
            // ring cells are written and read by this wave only: LDS operations of one wave complete in order
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            bad = __builtin_amdgcn_ballot_w64(gave) != 0;      // (no LDS round trip on the chain)
            if (prio_rim && !bad) __builtin_amdgcn_s_setprio(3);      // on the chain from here
        }
        // the rim wave looks at the slots once before its stress update -- the interior waves are usually done by the time the
        // neighbours' records have arrived -- so that the look's LDS round trip travels with the stress update's own loads
        int slots_seen = 0;
        if (rimw && !bad) {
            const int a0 = __hip_atomic_load(&s_slot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int a1 = __hip_atomic_load(&s_slot[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int a2 = __hip_atomic_load(&s_slot[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            slots_seen = __builtin_amdgcn_readfirstlane(min(a0, min(a1, a2))) >= done;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        EVP_STAMP(pacc0)
        if (prof && k == 0) lst4 = wall_clock64();      // (the rim wave: its first poll has matched; an interior wave: it starts)
        if (!bad) {      // (a wave whose wait gave up goes straight to the barrier)
            if (prio_in_stress) __builtin_amdgcn_s_setprio(1);
            if (actT) {
                double str[8];
                a.u_ij = s_u[li]; a.v_ij = s_v[li];
                a.u_im = s_u[li - 1]; a.v_im = s_v[li - 1];
                a.u_jm = s_u[li - LW]; a.v_jm = s_v[li - LW];
                a.u_mm = s_u[li - LW - 1]; a.v_mm = s_v[li - LW - 1];
                a.strength = s_tc[0 * 256 + t]; a.DminTarea = s_tc[1 * 256 + t];
                a.dxhy = s_tc[2 * 256 + t]; a.dyhx = s_tc[3 * 256 + t];
                MM::template stress<CAP, POL>(A.p, a, s, str, pol);
                s_str[0 * SP + sp] = str[2];
                s_str[1 * SP + sp] = str[5];
                s_str[2 * SP + sp] = str[3];
                s_str[3 * SP + sp] = str[7];
                s_str[4 * SP + sp] = str[1];
                s_str[5 * SP + sp] = str[6];
                s_str[6 * SP + sp] = str[0];
                s_str[7 * SP + sp] = str[4];
            }
            EVP_STAMP(pacc1)
            // the planes of this wave's T-cells are complete (s_waitcnt lgkmcnt(0)) before its slot says so; the rim wave's
            // are read by the rim wave only
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (!rimw && (t & 63) == 0) __hip_atomic_store(&s_slot[(tq >> 6) - 1], done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (prio_in_stress) __builtin_amdgcn_s_setprio(0);
            if (!slots_seen) {
                if (prio_rim) __builtin_amdgcn_s_setprio(0);
                unsigned spins = 0;
                for (;;) {
                    const int a0 = __hip_atomic_load(&s_slot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const int a1 = __hip_atomic_load(&s_slot[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const int a2 = __hip_atomic_load(&s_slot[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const int lo = __builtin_amdgcn_readfirstlane(min(a0, min(a1, a2)));
                    if (lo >= done) break;
                    if (++spins > R.spin_limit) {
                        give_up_note(5, k, -1, (unsigned)lo, (unsigned)done);
                        __hip_atomic_store(&s_bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    // (another wave of the tile gave up: nobody steps, everybody meets at the barrier)
                    if ((spins & 255u) == 0 || spins > R.spin_limit)
                        bad = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&s_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                    if (bad) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (prio_rim && !bad) __builtin_amdgcn_s_setprio(3);
            }
            if (prio_in_step && !bad) __builtin_amdgcn_s_setprio(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            EVP_STAMP(pacc2)
        }
        if (!bad) {
            double fin0 = 0.0, fin1 = 0.0, fin2 = 0.0, fin3 = 0.0;
            if constexpr (POL::lazy_taub) {
                // the same with the four outputs of the last subcycle formed where they are stored: strintx / strinty stay in
                // o (read under isU only, like the momentum step that sets them), taubx / tauby = -u * Cb, -v * Cb from the
                // operands stepu_post_cell forms them from
                typename MM::UO o;
                if (isU) {
                    typename MM::UI q;
                    ucell_operands(q);
                    q.sx0 = s_str[6 * SP + usp]; q.sx1 = s_str[4 * SP + usp + 1];
                    q.sx2 = s_str[0 * SP + usp + SW]; q.sx3 = s_str[2 * SP + usp + SW + 1];
                    q.sy0 = s_str[7 * SP + usp]; q.sy1 = s_str[1 * SP + usp + SW];
                    q.sy2 = s_str[5 * SP + usp + 1]; q.sy3 = s_str[3 * SP + usp + SW + 1];
                    if (!rimw) MM::template stepu_pre<CAP, false, POL>(A.p, q, upre, pol);
                    MM::template stepu_post<CAP, POL>(A.p, q, upre, o, pol);
                    u_own = o.u; v_own = o.v;
                }
                if (ownU) {      // the records first: the neighbours wait for them (every cell with a record to write is in L_U: rim_plan.h)
                    const unsigned tag = want + 1u;
                    if (pub) st_rec2_s(wr, own_off, pack_rec(u_own, tag), pack_rec(v_own, tag));
                    if (img0 >= 0) st_rec2_s(wr, img_off0, pack_rec(img_sg0 * u_own, tag), pack_rec(img_sg0 * v_own, tag));
                    if (img1 >= 0) st_rec2_s(wr, img_off1, pack_rec(img_sg1 * u_own, tag), pack_rec(img_sg1 * v_own, tag));
                    if (img2 >= 0) st_rec2_s(wr, img_off2, pack_rec(img_sg2 * u_own, tag), pack_rec(img_sg2 * v_own, tag));
                }
                if (prio_rim || prio_in_step) __builtin_amdgcn_s_setprio(0);      // off the chain
                if (isU) {
                    s_u[uli] = u_own; s_v[uli] = v_own;       // read by the next stress phase, after the barrier below
                    if (k == R.ndte - 1 && !R.dry) {
                        R.tab[24][cu] = o.strintx; R.tab[25][cu] = o.strinty;
                        R.tab[26][cu] = -u_own * upre.Cb; R.tab[27][cu] = -v_own * upre.Cb;
                    }
                }
            } else {
            if (isU) {
                typename MM::UI q;
                typename MM::UO o;
                ucell_operands(q);
                q.sx0 = s_str[6 * SP + usp]; q.sx1 = s_str[4 * SP + usp + 1];
                q.sx2 = s_str[0 * SP + usp + SW]; q.sx3 = s_str[2 * SP + usp + SW + 1];
                q.sy0 = s_str[7 * SP + usp]; q.sy1 = s_str[1 * SP + usp + SW];
                q.sy2 = s_str[5 * SP + usp + 1]; q.sy3 = s_str[3 * SP + usp + SW + 1];
                if (!rimw) MM::template stepu_pre<CAP, false, POL>(A.p, q, upre, pol);
                MM::template stepu_post<CAP, POL>(A.p, q, upre, o, pol);
                u_own = o.u; v_own = o.v;
                fin0 = o.strintx; fin1 = o.strinty; fin2 = o.taubx; fin3 = o.tauby;
            }
            if (ownU) {      // the records first: the neighbours wait for them (every cell with a record to write is in L_U: rim_plan.h)
                const unsigned tag = want + 1u;
                if (pub) st_rec2_s(wr, own_off, pack_rec(u_own, tag), pack_rec(v_own, tag));
                if (img0 >= 0) st_rec2_s(wr, img_off0, pack_rec(img_sg0 * u_own, tag), pack_rec(img_sg0 * v_own, tag));
                if (img1 >= 0) st_rec2_s(wr, img_off1, pack_rec(img_sg1 * u_own, tag), pack_rec(img_sg1 * v_own, tag));
                if (img2 >= 0) st_rec2_s(wr, img_off2, pack_rec(img_sg2 * u_own, tag), pack_rec(img_sg2 * v_own, tag));
            }
            if (prio_rim || prio_in_step) __builtin_amdgcn_s_setprio(0);      // off the chain
            if (isU) {
                s_u[uli] = u_own; s_v[uli] = v_own;       // read by the next stress phase, after the barrier below
                if (k == R.ndte - 1 && !R.dry) {
                    R.tab[24][cu] = fin0; R.tab[25][cu] = fin1;
                    R.tab[26][cu] = fin2; R.tab[27][cu] = fin3;
                }
            }
            }
            EVP_STAMP(pacc3)
        }
        __syncthreads();      // the one barrier: the tile's new velocities are in LDS, every read of the planes is done
        EVP_STAMP(pacc4)
        if (s_bad) return false;   // uniform: every thread of the workgroup leaves together
        // the rim wave's first part of the NEXT momentum step: after the barrier, where it runs while the neighbours' records are
        // still on their way (before the barrier it sat on the chain and measured slower: profiles/r14_resident_rim_u.txt, section 4)
        if (rimw && isU) {
            typename MM::UI q;
            ucell_operands(q);
            MM::template stepu_pre<CAP, false, POL>(A.p, q, upre, pol);
        }
        return true;
    };
    if constexpr (RIMU) {
        const v4u *const rec_a = (const v4u *)R.rec[par0 & 1];
        v4u *const rec_b = (v4u *)R.rec[(par0 & 1) ^ 1];
        for (int k = 0; k < R.ndte; k += 2) {
            if (!subcycle_rim(k, rec_a, rec_b)) return;
            if (k + 1 == R.ndte) break;
            if (!subcycle_rim(k + 1, rec_b, (v4u *)rec_a)) return;
        }
    } else
    if (LEAN) {
        // two subcycles per trip, one per record buffer: the buffers' addresses are fixed in each
        const v4u *const rec_a = (const v4u *)R.rec[par0 & 1];
        v4u *const rec_b = (v4u *)R.rec[(par0 & 1) ^ 1];
        for (int k = 0; k < R.ndte; k += 2) {
            if (!subcycle(k, rec_a, rec_b)) return;
            if (k + 1 == R.ndte) break;
            if (!subcycle(k + 1, rec_b, (v4u *)rec_a)) return;
        }
    } else {
        for (int k = 0; k < R.ndte; ++k)
            if (!subcycle(k, (const v4u *)R.rec[(k + par0) & 1], (v4u *)R.rec[((k + par0) & 1) ^ 1])) return;
    }
#undef EVP_STAMP
    unsigned long long lst5 = 0;
    EVP_LSTAMP(lst5)
    if (prof && (t & 63) == 0) {
        unsigned long long *o = R.prof + ((size_t)tile * 4 + (tq >> 6)) * 8;
        o[0] = pacc0; o[1] = pacc1; o[2] = pacc2; o[3] = pacc3; o[4] = pacc4;
        o[5] = (unsigned long long)cu_rank | ((unsigned long long)(PERM && R.cuload ? s_cu : 0) << 8) | ((unsigned long long)(s_simd[t >> 6] & 3) << 24);
        unsigned long long nlib = 0;      // passes of this wave that took the compiler's sqrt / division (evp_range_math.h)
        if constexpr (POL::ranged) nlib = pol.nlib;
        o[6] = (unsigned long long)(t >> 6) | (nlib << 8); o[7] = (unsigned long long)R.nact[tile];
    }
    // ghost cells that mirror another rank's cells: fetch the final velocities (the caller
    // relies on current ghosts, ice_dyn_evp.F90:920-934)
    if (REMOTE && ring_remote) {
        v4u ra, rb;
        const v4u *rd = (const v4u *)R.rec[(R.ndte + par0) & 1];
        const bool ok = poll_remote(rd + 2 * (size_t)ring_cp, R.tag_base + (unsigned)R.ndte, ra, rb);
        if (ok && !R.dry) {
#pragma unroll
            for (int b = 0; b < 2; ++b) { R.u[b][ring_cp] = unpack_rec(ra); R.v[b][ring_cp] = unpack_rec(rb); }
        }
    }

    // ---- write the state back --------------------------------------------------------------
    // LEAN, one store per value: into the ping-pong buffer that is current after the call, cur0 ^ (ndte & 1) -- the one the host's
    // S.cur names from here on.  That is how every call of the streaming kernel leaves the two buffers (its last subcycle writes
    // the ice T-cells' stresses and the ice U-cells' velocities with their images into one of them, evp_kernels.hip): they differ
    // on cells the loop writes and nowhere else.  Every reader -- the download, the stress halo, the tail, the preparation, the
    // marching and streaming kernels, the next resident launch, the replay snapshot -- reads the current buffer, and every kernel
    // that advances the state writes those very cells of the other buffer before anybody reads them; off the masks the buffers
    // stay equal (the upload copies, evp_launch_zero_sig_off_mask zeroes both).  The product compiles it in or out
    // (EVP_RES2_WRITE_ONCE_DEFAULT); the test build carries a switch (EVP_RES2_HOOK_WRITE_ONCE, CICE_EVP_HIP_RES_WRITE_ONCE).
#ifdef CICE_EVP_HIP_TESTING
    const bool write_once = LEAN && (RES_DBG(R) & EVP_RES2_HOOK_WRITE_ONCE);
#else
    constexpr bool write_once = LEAN && EVP_RES2_WRITE_ONCE_DEFAULT;
#endif
    if (write_once) {
        if (!R.dry) {
            const int fin = (R.cur0 ^ (R.ndte & 1)) & 1;
            if (actN && own) {
#pragma unroll
                for (int k = 0; k < 12; ++k) R.tab[fin * 12 + k][c] = s[k];
            }
            if (isU) {
                double *uu = R.u[fin], *vv = R.v[fin];
                uu[cu] = u_own; vv[cu] = v_own;
                if (img0 >= 0) { uu[img0 >> 1] = img_sg0 * u_own; vv[img0 >> 1] = img_sg0 * v_own; }
                if (img1 >= 0) { uu[img1 >> 1] = img_sg1 * u_own; vv[img1 >> 1] = img_sg1 * v_own; }
                if (img2 >= 0) { uu[img2 >> 1] = img_sg2 * u_own; vv[img2 >> 1] = img_sg2 * v_own; }
            }
        }
    } else
    if (!R.dry) {
        if (actN && own) {
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                R.tab[k][c] = s[k];
                R.tab[12 + k][c] = s[k];
            }
        }
        if (quad && gown) {
            R.tab[qc][gc] = sr0; R.tab[12 + qc][gc] = sr0;
            R.tab[4 + qc][gc] = sr1; R.tab[16 + qc][gc] = sr1;
            R.tab[8 + qc][gc] = sr2; R.tab[20 + qc][gc] = sr2;
        }
        if (isU || isSeam) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                double *uu = R.u[b], *vv = R.v[b];
                uu[cu] = u_own; vv[cu] = v_own;
                if (img0 >= 0) { const double sg = (img0 & 1) ? -1.0 : 1.0; uu[img0 >> 1] = sg * u_own; vv[img0 >> 1] = sg * v_own; }
                if (img1 >= 0) { const double sg = (img1 & 1) ? -1.0 : 1.0; uu[img1 >> 1] = sg * u_own; vv[img1 >> 1] = sg * v_own; }
                if (img2 >= 0) { const double sg = (img2 & 1) ? -1.0 : 1.0; uu[img2 >> 1] = sg * u_own; vv[img2 >> 1] = sg * v_own; }
            }
        }
    }
    if (RES_PROF(R)) {
        unsigned long long lst6 = 0;
        EVP_LSTAMP(lst6)
        if ((t & 63) == 0) {      // per wave as it was dispatched, behind the [ntiles][4][8] phase stamps
            unsigned long long *o = R.prof + ((size_t)A.ntiles * 4 + (size_t)tile * 4 + (t >> 6)) * 8;
            o[0] = lst0; o[1] = lst1; o[2] = lst2; o[3] = lst3; o[4] = lst4; o[5] = lst5; o[6] = lst6;
            o[7] = (unsigned long long)(tq >> 6) | ((unsigned long long)R.nact[tile] << 8);
        }
    }
#undef EVP_LSTAMP
}

size_t lds_bytes(const Res2Variant &v, unsigned flags)
{
    const int W = 1 << v.logw, H = 256 / W;
    const int nuv = ((H + 1) * (W + 1) + 7) & ~7;
    const int nu = 8 + ((flags & EVP_F_WATER_IS_OCN) ? 0 : 2) + ((flags & EVP_F_TBU_ZERO) ? 0 : 1);
    const size_t nstr = v.logw == 4 ? (v.rimu ? 8 : 6) * (size_t)(W + 1) * H : 4 * (size_t)256;   // PERM planes: row stride W + 1 (RIMU: eight of them)
    return sizeof(double) * (nstr + (size_t)256 * (4 + nu) + 2 * (size_t)nuv + (v.coop ? 12 * (size_t)64 : 0));
}

// ---- the table of instantiations (this template and evp_resident2_kernel below): the launch, the occupancy query and "is it
// built" all ask it.  General: {strict} x {cap 3, 1, 0, -1} x {logw 4, 5, 6} x {remote}
#define EVP_TILE(...) ((const void *)evp_resident2_tile<__VA_ARGS__>)
template <int LOGW, bool REMOTE>
const void *general_tile(bool strict, int cap)
{
    if (strict) return cap == 3 ? EVP_TILE(true, 3, LOGW, REMOTE) : cap == 1 ? EVP_TILE(true, 1, LOGW, REMOTE) : cap == 0 ? EVP_TILE(true, 0, LOGW, REMOTE) : cap == -1 ? EVP_TILE(true, -1, LOGW, REMOTE) : nullptr;
    return cap == 3 ? EVP_TILE(false, 3, LOGW, REMOTE) : cap == 1 ? EVP_TILE(false, 1, LOGW, REMOTE) : cap == 0 ? EVP_TILE(false, 0, LOGW, REMOTE) : cap == -1 ? EVP_TILE(false, -1, LOGW, REMOTE) : nullptr;
}

}  // namespace

#ifdef CICE_EVP_HIP_TESTING
// Test build: the cores of evp_range_math.h beside the compiler's sqrt and division, element by element, with the verdicts of the
// window tests the kernels use (cice_evp_hip_debug_range_math, tests/test_gpu_range_math.py).  Device pointers, n elements each.
namespace {
__global__ __launch_bounds__(256) void range_math_probe(long long n, const double *x, const double *num, const double *den, double *sqrt_lib,
                                                        double *sqrt_core, double *div_lib, double *div_core, unsigned char *verdict)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double xx = x[e], nn = num[e], dd = den[e];
    sqrt_lib[e] = sqrt(xx);
    sqrt_core[e] = evp_range::sqrt_core(xx);
    div_lib[e] = nn / dd;
    div_core[e] = evp_range::div_core(nn, dd);
    const bool x_in = !evp_range::outside(evp_range::off_pos(xx));
    const bool q_in = !evp_range::outside(evp_range::umax(evp_range::off_abs(nn), evp_range::off_abs(dd)));
    verdict[e] = (unsigned char)((x_in ? 1 : 0) | (q_in ? 2 : 0));
}
}  // namespace
hipError_t evp_range_math_probe(long long n, const double *x, const double *num, const double *den, double *sqrt_lib, double *sqrt_core,
                                double *div_lib, double *div_core, unsigned char *verdict, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(range_math_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x, num, den, sqrt_lib, sqrt_core, div_lib,
                       div_core, verdict);
    return hipGetLastError();
}
#endif

void evp_resident_geometry(int max_ni, int max_nj, int logw, int *gx, int *gy)
{
    const int W = 1 << logw, H = 256 / W;
    *gx = (max_ni + W - 2) / (W - 1);
    *gy = (max_nj + H - 2) / (H - 1);
}

// Coop (test build): strict, cap 3, logw 4, not remote; lean and lean + rimu: cap 3, logw 4, not remote.  (The kernels are named in
// the order the file has always instantiated them: the compiler lays the code object out in it, and that layout is what was measured.)
const void *evp_resident2_kernel(const Res2Variant &v)
{
    if (v.coop || v.lean || v.rimu) {
        if (v.cap != 3 || v.logw != 4 || v.remote) return nullptr;
#ifdef CICE_EVP_HIP_TESTING
        if (v.coop) return v.strict && !v.lean && !v.rimu ? EVP_TILE(true, 3, 4, false, true) : nullptr;
#endif
        if (v.coop || !v.lean) return nullptr;
        if (!v.rimu) return v.strict ? EVP_TILE(true, 3, 4, false, false, true) : EVP_TILE(false, 3, 4, false, false, true);
        return v.strict ? EVP_TILE(true, 3, 4, false, false, true, true) : EVP_TILE(false, 3, 4, false, false, true, true);
    }
    if (v.logw == 4 && !v.remote) return general_tile<4, false>(v.strict, v.cap);
    if (v.remote) return v.logw == 4 ? general_tile<4, true>(v.strict, v.cap) : v.logw == 5 ? general_tile<5, true>(v.strict, v.cap) : v.logw == 6 ? general_tile<6, true>(v.strict, v.cap) : nullptr;
    return v.logw == 5 ? general_tile<5, false>(v.strict, v.cap) : v.logw == 6 ? general_tile<6, false>(v.strict, v.cap) : nullptr;
}
#undef EVP_TILE

int evp_resident2_max_blocks_per_cu(const Res2Variant &v, unsigned flags)
{
    auto occ = [](const Res2Variant &w, unsigned fl) {
        const void *k = evp_resident2_kernel(w);
        int nb = 0;
        return k && hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 64 * RTY, lds_bytes(w, fl)) == hipSuccess ? nb : 0;
    };
    Res2Variant lean = v, rimu = v;
    lean.lean = rimu.lean = rimu.rimu = true;
    if (v.coop || v.lean || !evp_resident2_kernel(lean)) return occ(v, flags);
    // admitted against the smallest of the three: the launch picks the lean variants only while the data allow it (RIMU: two more
    // planes, 46720 B of LDS per workgroup with the operands the lean launch has)
    return std::min(std::min(occ(lean, flags), occ(rimu, flags | EVP_F_WATER_IS_OCN | EVP_F_TBU_ZERO)), occ(v, flags));
}

hipError_t evp_launch_resident2(const EvpArgs &A0, const EvpResident2 &R, int max_ni, int max_nj, const Res2Variant &v, hipStream_t st)
{
    const void *kernel = evp_resident2_kernel(v);
    if (!kernel) return hipErrorInvalidDeviceFunction;
    EvpArgs A = A0;
    evp_resident_geometry(max_ni, max_nj, v.logw, &A.gx, &A.gy);
    A.ntiles = A.gx * A.gy * (R.nblocks > 0 ? R.nblocks : 1);
    void *args[2] = {&A, const_cast<EvpResident2 *>(&R)};
    return hipLaunchKernel(kernel, dim3(R.nlaunch > 0 ? R.nlaunch : A.ntiles), dim3(64, RTY), args, lds_bytes(v, A.flags), st);
}
