"""GPU (-m gpu), one rank: the passes between the last subcycle and transport on the device (cice_evp_hip_cgrid_tail,
cice_evp_hip_strocn_t / _cgrid_strocn_t, cice_evp_hip_principal_stress) against the reference's own arrays where a fixture holds
them and against tests/tail_ref.py (numpy fp64 in the reference's order of operations) everywhere else -- by bit pattern in both
build modes: the kernels of these passes are compiled without FMA contraction whichever build ran the loop."""
import numpy as np
import pytest

import oracle
import tail_ref
from cice_amd import decomp, evp, synth
from common import CGRID_CASES, CGRID_TFOLD_CASES, GOLDEN_CASES, TFOLD_CASES, GoldenCase, assert_bitwise, bits_equal
from test_gpu_cgrid import cgrid_core, synth_cgrid
from test_gpu_parity import hip_from_case

pytestmark = pytest.mark.gpu

PUNY = 1.0e-11          # icepack's puny
TAIL_KEYS = ("strintxE", "strintyN", "strintxU", "strintyU")


def ghost(shape, blocks):
    return ~tail_ref._interior(shape, blocks)


def top_rows(c_or_dc, blocks, ny_global, jglob):
    """[(block, row index)] of the top physical row of the grid."""
    return [(b, jhi - 1) for b, (ilo, ihi, jlo, jhi) in enumerate(blocks) if jglob[b] + (jhi - jlo) == ny_global]


# ---- the end of evp() on the C grid -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CGRID_CASES + CGRID_TFOLD_CASES)
def test_cgrid_tail_on_the_fixtures(name):
    """cgrid_run, then cgrid_tail(): strintxE / strintyN equal the arrays the reference's evp() left, bit for bit on every cell,
    with NO halo update on the host; strintxU / strintyU equal the restatement and are 0 on every ghost cell; cgrid_download
    afterwards returns the updated arrays."""
    c = GoldenCase(name)
    dom, blocks, static = c.oracle_domain(), tail_ref.blocks_of(c), c.cgrid_static()
    core = cgrid_core(c)
    moved = False
    try:
        for icall in range(1, c.ncalls + 1):
            state, inputs, masks = c.cgrid_inputs(icall)
            for nsub in c.nsub_list:
                what = f"{name} call {icall} nsub {nsub}"
                loop = core.cgrid_run(nsub, state, inputs, masks, visc_method=str(c.d["visc_method"]))
                got = core.cgrid_tail()
                want = c.cgrid_expected(icall, nsub)
                assert_bitwise({k: got[k] for k in TAIL_KEYS[:2]}, {k: want[k] for k in TAIL_KEYS[:2]}, f"{what}: cgrid_tail vs the reference")
                moved = moved or not bits_equal(loop["strintxE"], want["strintxE"]) or not bits_equal(loop["strintyN"], want["strintyN"])
                ref = tail_ref.cgrid_tail(dom, blocks, loop["strintxE"], loop["strintyN"], static)
                assert_bitwise(got, ref, f"{what}: cgrid_tail vs tail_ref")
                gh = ghost(got["strintxU"].shape, blocks)
                for k in TAIL_KEYS[2:]:
                    assert bits_equal(got[k][gh], np.zeros(int(gh.sum()))), f"{what}: {k} is not +0 on every ghost cell"
                assert_bitwise(core.cgrid_download(), want, f"{what}: cgrid_download after the tail")
        assert np.abs(got["strintxU"]).max() > 0 and np.abs(got["strintyU"]).max() > 0
        assert moved, "the loop's own strintxE / strintyN already equal the reference's on every ghost cell"
    finally:
        core.finalize()


def dilated_halomask(dom, blocks, iceT):
    """evp()'s halo mask for the C grid: the five-point dilation of iceTmask, ghost cells updated (ice_dyn_evp.F90:739-770)."""
    t = oracle.halo_update(dom, (iceT != 0).astype(np.float64), "center", "scalar")
    m = np.zeros_like(t)
    m[:, 1:-1, 1:-1] = np.maximum.reduce([t[:, 1:-1, 1:-1], t[:, :-2, 1:-1], t[:, 2:, 1:-1], t[:, 1:-1, :-2], t[:, 1:-1, 2:]])
    m *= tail_ref._interior(t.shape, blocks)
    return (oracle.halo_update(dom, m, "center", "scalar") != 0).astype(np.int32)


def test_cgrid_tail_ignores_a_masked_halo(monkeypatch):
    """maskhalo_dyn: the loop's exchanges run over the masked lists, the tail's over the plain ones.  Caps cover on 30 x 40 blocks,
    every ghost copy routed through the exchange (the rank with itself); strintxE / strintyN are handed over with a sentinel in
    every ghost cell, which a masked exchange would leave standing wherever the mask is 0."""
    monkeypatch.setenv("CICE_EVP_HIP_SELF_EXCHANGE", "1")
    monkeypatch.setenv("CICE_EVP_HIP_HALO", "rccl")
    dc, g, static, state, inputs, masks = synth_cgrid("gx3", case="caps", bs=(30, 40))
    dom, blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
    gh = ghost(state["strintxE"].shape, blocks)
    state = dict(state)
    for k in ("strintxE", "strintyN"):
        state[k] = np.where(gh, 7.25, state[k])
    scal = synth.evp_scalars(120)
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"], 1.0 / static["uarea"],
                      static["tarea"], keepalive=keep)
    try:
        core.comm_init(core.comm_unique_id())
        core.cgrid_set_geometry(static)
        full = core.timings()["halo_send_cells"]
        hm = dilated_halomask(dom, blocks, masks["iceTmask"])
        core.halo_mask(hm)
        assert 0 < core.timings()["halo_send_cells"] < full
        loop = core.cgrid_run(8, state, inputs, masks)
        got = core.cgrid_tail()
        ref = tail_ref.cgrid_tail(dom, blocks, loop["strintxE"], loop["strintyN"], static)
        assert_bitwise(got, ref, "cgrid_tail with a masked halo handed over")
        # ghost cells off the mask that ice_HaloUpdate writes (every one but those outside the closed north-south boundary)
        stale = gh & (hm == 0) & (loop["strintxE"] == 7.25) & (ref["strintxE"] != 7.25)
        assert stale.any() and not (got["strintxE"][stale] == 7.25).any(), "no ghost cell off the mask shows that the full lists ran"
        outer = gh & (ref["strintxE"] == 7.25)
        assert outer.any() and (got["strintxE"][outer] == 7.25).all()       # ... which keep what they held, as in the reference
        assert np.abs(got["strintxU"]).max() > 0
    finally:
        core.finalize()


def u_point_inputs(shape, iceU, seed):
    """U-point operands of dyn_finish for a C-grid case (the loop holds none): any numbers do."""
    rng = np.random.default_rng(seed)
    ai = np.where(iceU != 0, rng.uniform(0.2, 1.0, shape), np.where(rng.uniform(size=shape) < 0.5, 0.0, 1e-12))
    return dict(cdn_ocnU=np.full(shape, 0.00536), aiU=ai, uocnU=rng.uniform(-0.1, 0.1, shape), vocnU=rng.uniform(-0.1, 0.1, shape),
                fmU=rng.uniform(-20.0, 20.0, shape))


@pytest.mark.parametrize("name", CGRID_CASES + CGRID_TFOLD_CASES)
def test_cgrid_strocn_t_on_the_fixtures(name):
    """cgrid_run -> cgrid_dyn_finish_u -> cgrid_strocn_t: dyn_finish at U points equals the oracle's on the reference's final uvel /
    vvel; strocn{x,y}T_iavg equals the restatement from those arrays."""
    c = GoldenCase(name)
    dom, blocks, static, prm = c.oracle_domain(), tail_ref.blocks_of(c), c.cgrid_static(), c.oracle_params()
    core = cgrid_core(c)
    try:
        state, inputs, masks = c.cgrid_inputs(1)
        nsub = c.nsub_list[-1]
        core.cgrid_run(nsub, state, inputs, masks, visc_method=str(c.d["visc_method"]))
        want = c.cgrid_expected(1, nsub)
        uin = u_point_inputs(want["uvel"].shape, masks["iceUmask"], seed=17)
        z = np.zeros_like(want["uvel"])
        fin = core.cgrid_dyn_finish_u(uin)
        sx, sy = oracle.dyn_finish_at(dom, prm, uin["cdn_ocnU"], uin["aiU"], uin["uocnU"], uin["vocnU"], uin["fmU"], want["uvel"], want["vvel"],
                                      masks["iceUmask"], z, z)
        assert_bitwise(fin, dict(strocnxU=sx, strocnyU=sy), f"{name}: dyn_finish at U points")
        got = core.cgrid_strocn_t()
        ref = tail_ref.strocn_t(dom, blocks, sx, sy, uin["aiU"], static["uarea"], static["tarea"])
        assert_bitwise(got, ref, f"{name}: cgrid_strocn_t")
        assert np.abs(got["strocnxT_iavg"]).max() > 0 and np.abs(got["strocnyT_iavg"]).max() > 0
        if c.ns in ("tripole", "tripoleT"):
            nofold = tail_ref.strocn_t(oracle.OracleDomain.from_dump(c.d, c.ew, "closed"), blocks, sx, sy, uin["aiU"], static["uarea"], static["tarea"])
            rows = top_rows(c, blocks, c.ny_global, c.blk[:, 7])
            assert any(not bits_equal(got["strocnxT_iavg"][b, j], nofold["strocnxT_iavg"][b, j]) for b, j in rows), "the fold changed nothing"
    finally:
        core.finalize()


def test_cgrid_tail_calls_fail_loudly_out_of_order():
    c = GoldenCase(CGRID_CASES[0])
    core = cgrid_core(c)
    try:
        with pytest.raises(evp.EvpHipError, match="nothing uploaded"):
            core.cgrid_tail()
        state, inputs, masks = c.cgrid_inputs(1)
        core.cgrid_run(1, state, inputs, masks, visc_method=str(c.d["visc_method"]))
        with pytest.raises(evp.EvpHipError, match="cgrid_dyn_finish_u first"):
            core.cgrid_strocn_t()
    finally:
        core.finalize()


# ---- the T-point ocean stress on the B grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES + TFOLD_CASES)
def test_strocn_t_on_the_fixtures(name):
    """upload -> subcycle -> dyn_finish -> strocn_t against the restatement from the fixture's own strocnxU / strocnyU (the
    reference's evp() output), aiU, uarea, tarea; on a fold the top physical row must differ from a run without the fold step."""
    c = GoldenCase(name)
    dom, blocks = c.oracle_domain(), tail_ref.blocks_of(c)
    core = hip_from_case(c, strict=True)
    try:
        with pytest.raises(evp.EvpHipError, match="upload"):
            core.strocn_t(c.d["uarea"], c.d["tarea"])
        for icall in range(1, c.ncalls + 1):
            dyn, tm, um = c.inputs(icall)
            nsub = c.nsub_list[-1]
            core.upload(dyn, tm, um)
            core.subcycle(nsub)
            if icall == 1:
                with pytest.raises(evp.EvpHipError, match="dyn_finish first"):
                    core.strocn_t(c.d["uarea"], c.d["tarea"])
            z = np.zeros(core.shape)
            fin = core.dyn_finish(z, z)
            key = f"o{icall:02d}n{nsub:04d}_strocnxU"
            sx, sy = (c.d[key], c.d[key.replace("xU", "yU")]) if key in c.d else (fin["strocnxU"], fin["strocnyU"])
            got = core.strocn_t(c.d["uarea"], c.d["tarea"]) if icall == 1 else core.strocn_t()
            ref = tail_ref.strocn_t(dom, blocks, sx, sy, dyn["aiU"], c.d["uarea"], c.d["tarea"])
            assert_bitwise(got, ref, f"{name} call {icall}: strocn_t")
            gh = ghost(core.shape, blocks)
            assert bits_equal(got["strocnxT_iavg"][gh], np.zeros(int(gh.sum())))
            assert np.abs(got["strocnxT_iavg"]).max() > 0 and np.abs(got["strocnyT_iavg"]).max() > 0
            if c.ns in ("tripole", "tripoleT"):
                nofold = tail_ref.strocn_t(oracle.OracleDomain.from_dump(c.d, c.ew, "closed"), blocks, sx, sy, dyn["aiU"], c.d["uarea"], c.d["tarea"])
                rows = top_rows(c, blocks, c.ny_global, c.blk[:, 7])
                assert any(not bits_equal(got["strocnxT_iavg"][b, j], nofold["strocnxT_iavg"][b, j]) for b, j in rows), "the fold changed nothing"
    finally:
        core.finalize()


class SmallCase:
    """A small synthetic B-grid case through cice_amd/synth.py and decomp.py: the loop's inputs on an nx x ny grid cut into blocks,
    optionally with one block eliminated (its cells are land).  tripoleT: the u-fold's grid under the T-fold halo rule, velocities
    handed over with the top row as the fold's image, dxhy / dyhx as oracle.metrics leaves them (tests/evp_call_chain.py)."""

    def __init__(self, nx, ny, bs, ew, ns, cover, drop=None, seed=20261020):
        grid = synth.make_grid(nx, ny, 1.1e5, ns=("tripole" if ns == "tripoleT" else ns))
        self.dc = dc = decomp.Decomp(nx, ny, bs[0], bs[1], ew, ns, 1)
        dropped = np.zeros((ny, nx))
        if drop:
            for b in dc.blocks:
                if (b.iblock, b.jblock) == drop:
                    b.owner = -1
                    grid["kmt"][b.gj0 - 1:b.gj0 - 1 + b.gny, b.gi0 - 1:b.gi0 - 1 + b.gnx] = 0
                    dropped[b.gj0 - 1:b.gj0 - 1 + b.gny, b.gi0 - 1:b.gi0 - 1 + b.gnx] = 1.0
            for k, b in enumerate(sorted((b for b in dc.blocks if b.owner == 0), key=lambda b: b.gid)):
                b.local = k
        g = synth.derive_geometry(grid)
        st = synth.make_state(g, case=cover, seed=seed, warm=True)
        if ns == "tripoleT":
            for k in ("uvel", "vvel", "uvel_init", "vvel_init"):
                st[k] = np.array(st[k], dtype=np.float64, copy=True)
                st[k][ny - 1, :] = -st[k][ny - 2, ::-1]
        sc = lambda a, fill=0.0: dc.scatter(np.ascontiguousarray(a), 0, fill=fill)
        self.geo = {k: sc(g[k], 1.0 if k != "uarear" else 0.0) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear", "uarea")}
        self.dom, self.blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
        # ghost cells whose source lies in the eliminated block (tail_ref.strocn_t: the fill value 0 there)
        self.land_ghosts = (dc.scatter(dropped, 0) != 0) if drop else None
        self.dom_nofold = tail_ref.domain_of_decomp(dc, ns="closed")
        self.scal = synth.evp_scalars(120)
        self.fold_metrics = None
        if ns == "tripole":
            self.fold_metrics = synth.bgrid_fold_metrics(dc, 0, g)
        elif ns == "tripoleT":
            m = oracle.metrics(self.dom, self.scal["deltaminEVP"], self.geo["HTE"], self.geo["HTN"], self.geo["tarea"])
            self.fold_metrics = (m["dxhy"], m["dyhx"])
        self.dyn = {k: sc(st[k]) for k in evp.FIELDS}
        self.tm, self.um = dc.scatter(st["iceTmask"], 0, fill=0), dc.scatter(st["iceUmask"], 0, fill=0)
        self.jglob = [b.gj0 for b in dc.local_blocks(0)]

    def open_core(self, strict=True):
        d, keep = evp.make_dims(self.dc, 0)
        g = self.geo
        core = evp.EvpHip(d, evp.make_params(self.scal, strict=strict), g["HTE"], g["HTN"], g["dxT"], g["dyT"], g["uarear"], g["tarea"], keepalive=keep)
        if self.fold_metrics is not None:
            core.set_metrics(dxhy=self.fold_metrics[0], dyhx=self.fold_metrics[1])
        return core


SMALL = {
    "48x32 closed, 2x2 blocks of 24x16": (48, 32, (24, 16), "closed", "closed", None),
    "48x32 tripole, padded blocks of 20x12": (48, 32, (20, 12), "cyclic", "tripole", None),
    "72x40 tripoleT, blocks of 18x10, one land block eliminated": (72, 40, (18, 10), "cyclic", "tripoleT", (2, 2)),
}


@pytest.mark.parametrize("cover", ["caps", "full"])
@pytest.mark.parametrize("case", list(SMALL))
def test_strocn_t_small_synthetic_cases(case, cover):
    nx, ny, bs, ew, ns, drop = SMALL[case]
    s = SmallCase(nx, ny, bs, ew, ns, cover, drop)
    core = s.open_core()
    try:
        core.upload(s.dyn, s.tm, s.um)
        core.subcycle(12)
        # The synthetic grids have no ice U-cell on the top row (land beyond it), so the u-fold's top-row averaging would see zeros
        # only: dyn_finish's arrays are inout, and the top row is handed in with numbers, which it keeps off the ice
        rng = np.random.default_rng(3)
        prev = [np.zeros(core.shape), np.zeros(core.shape)]
        for b, j in top_rows(s.dc, s.blocks, ny, s.jglob):
            ilo, ihi = s.blocks[b][:2]
            for p in prev:
                p[b, j, ilo - 1:ihi] = rng.uniform(-1.0, 1.0, ihi - ilo + 1)
        fin = core.dyn_finish(*prev)
        got = core.strocn_t(s.geo["uarea"], s.geo["tarea"])
        ref = tail_ref.strocn_t(s.dom, s.blocks, fin["strocnxU"], fin["strocnyU"], s.dyn["aiU"], s.geo["uarea"], s.geo["tarea"],
                                land_ghosts=s.land_ghosts)
        assert_bitwise(got, ref, f"{case}, {cover}: strocn_t")
        assert np.abs(fin["strocnxU"]).max() > 0 and np.abs(got["strocnxT_iavg"]).max() > 0 and np.abs(got["strocnyT_iavg"]).max() > 0
        if ns != "closed":
            nofold = tail_ref.strocn_t(s.dom_nofold, s.blocks, fin["strocnxU"], fin["strocnyU"], s.dyn["aiU"], s.geo["uarea"], s.geo["tarea"],
                                       land_ghosts=s.land_ghosts)
            rows = top_rows(s.dc, s.blocks, ny, s.jglob)
            assert rows and any(not bits_equal(got["strocnxT_iavg"][b, j], nofold["strocnxT_iavg"][b, j]) for b, j in rows), "the fold changed nothing"
        # the second call keeps uarea / tarea
        assert_bitwise(core.strocn_t(), ref, f"{case}, {cover}: strocn_t again, areas kept")
    finally:
        core.finalize()


def test_same_bits_whichever_loop_path_ran(monkeypatch):
    """Streaming kernel, on-chip resident kernel, marching kernel (forced at gx3 size, as tests/test_gpu_march.py does): the calls
    after the loop read the state each path leaves in its own way and return the same bits; so does the fused build against the
    restatement applied to ITS loop's outputs (the passes are not contracted), while its numbers differ from the strict build's."""
    from evp_call_chain import assert_path_ran, set_path, synth_case
    case = synth_case("closed holes 30x40")
    ndte = 9
    uarea = case.dc.scatter(np.ascontiguousarray(synth.derive_geometry(synth.make_grid(100, 116, 3.3e5, ns="closed"))["uarea"]), 0, fill=1.0)
    first = None
    for path, strict in (("streaming", True), ("resident general", True), ("marching k=4", True), ("streaming", False)):
        set_path(monkeypatch, path)
        core = case.open_core(strict=strict)
        try:
            loop = case.device_loop(core, ndte)
            assert_path_ran(core, path, ndte, False, None, f"{path}")
            prin = core.principal_stress(PUNY)
            z = np.zeros(core.shape)
            fin = core.dyn_finish(z, z)
            got = core.strocn_t(uarea, case.geo["tarea"])
        finally:
            core.finalize()
        ref = tail_ref.strocn_t(case.dom, case.blocks, fin["strocnxU"], fin["strocnyU"], case.dyn["aiU"], uarea, case.geo["tarea"])
        assert_bitwise(got, ref, f"strocn_t after {path}, strict={strict}")
        assert_bitwise(prin, tail_ref.principal_stress(loop["stressp_1"], loop["stressm_1"], loop["stress12_1"], case.dyn["strength"], PUNY),
                       f"principal_stress after {path}, strict={strict}")
        if first is None:
            first = (got, prin)
        elif strict:
            assert_bitwise(got, first[0], f"strocn_t: {path} vs streaming")
            assert_bitwise(prin, first[1], f"principal_stress: {path} vs streaming")
        else:
            assert not bits_equal(got["strocnxT_iavg"], first[0]["strocnxT_iavg"]), "the fused build's loop gave the strict build's bits"
            scale = np.abs(first[0]["strocnxT_iavg"]).max()
            assert np.abs(got["strocnxT_iavg"] - first[0]["strocnxT_iavg"]).max() < 1e-9 * scale


# ---- principal stresses -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pop_cyc_2x2_cap05", "trip_cyc_2x2_full"])
def test_principal_stress_on_fixtures(name):
    c = GoldenCase(name)
    core = hip_from_case(c, strict=True)
    try:
        dyn, tm, um = c.inputs(1)
        core.upload(dyn, tm, um)
        core.subcycle(c.ndte)
        if c.ns == "tripole":
            core.stress_halo()
        got = core.principal_stress(PUNY)
        want = c.expected(1, c.ndte)                 # (the state after the whole evp(), symmetrisation included)
        ref = tail_ref.principal_stress(want["stressp_1"], want["stressm_1"], want["stress12_1"], dyn["strength"], PUNY)
        assert_bitwise(got, ref, f"{name}: principal_stress")
        on = dyn["strength"] > PUNY
        assert on.any() and (~on).any() and (got["sig1"][~on] == 1.0e30).all() and np.abs(got["sig1"][on]).max() > 0
        assert_bitwise(core.download(), want, f"{name}: the download after principal_stress")
    finally:
        core.finalize()


def test_principal_stress_at_the_threshold():
    """strength exactly puny, one ulp above it, and 0 on cells that carry stress: the first and the last take spval_dbl."""
    c = GoldenCase("pop_cyc_2x2_cap05")
    core = hip_from_case(c, strict=True)
    try:
        dyn, tm, um = c.inputs(1)
        dyn = dict(dyn)
        b0 = tail_ref.blocks_of(c)
        cells = np.argwhere((tm != 0) & (dyn["strength"] > 1.0) & tail_ref._interior(tm.shape, b0))[:9]
        assert len(cells) == 9
        st = np.array(dyn["strength"], copy=True)
        for q, (b, j, i) in enumerate(cells):
            st[b, j, i] = (PUNY, np.nextafter(PUNY, 1.0), 0.0)[q % 3]
        dyn["strength"] = st
        core.upload(dyn, tm, um)
        core.subcycle(1)
        got = core.principal_stress(PUNY)
        loop = core.download()
        ref = tail_ref.principal_stress(loop["stressp_1"], loop["stressm_1"], loop["stress12_1"], st, PUNY)
        assert_bitwise(got, ref, "principal_stress at the threshold")
        for q, (b, j, i) in enumerate(cells):
            assert (got["sig1"][b, j, i] == 1.0e30) == (q % 3 != 1) and (got["sigP"][b, j, i] == 1.0e30) == (q % 3 != 1)
        assert any(loop["stressp_1"][b, j, i] != 0 for b, j, i in cells), "none of the chosen cells carries stress"
    finally:
        core.finalize()


def test_principal_stress_with_resident_stresses():
    """CICE_EVP_HIP_OPT_STRESS_RESIDENT: cice_evp_hip_run writes no stress back; principal_stress reads them where they are."""
    c = GoldenCase("pop_cyc_2x2_cap05")
    core = hip_from_case(c, strict=True)
    try:
        core.set_option(evp.OPT_STRESS_RESIDENT, 1)
        dyn, tm, um = c.inputs(1)
        out = core.run(dyn, tm, um, ndte=c.ndte)
        assert bits_equal(out["stressp_1"], dyn["stressp_1"]), "the stresses came back although they are resident"
        got = core.principal_stress(PUNY)
        want = c.expected(1, c.ndte)
        assert not bits_equal(want["stressp_1"], dyn["stressp_1"])
        assert_bitwise(got, tail_ref.principal_stress(want["stressp_1"], want["stressm_1"], want["stress12_1"], dyn["strength"], PUNY),
                       "principal_stress from resident stresses")
    finally:
        core.finalize()
