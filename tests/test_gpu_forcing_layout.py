"""The preparation phase of evp() on the device under every forcing layout the reference accepts
(cice_evp_hip_set_forcing_layout): the ocean on grid A / B / C, the wind stress computed by CICE (calc_strair) or given as
strax / stray on grid A / B / C -- on the B grid and on the C grid.  Pinned on the committed fixtures by layouts that must
reproduce the default's bits, and compared layout by layout with the numpy restatement (tests/forcing_layout_ref.py)."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from cice_amd import decomp, evp, synth
from common import CGRID_CASES, CGRID_TFOLD_CASES, GOLDEN_CASES, TFOLD_CASES, GoldenCase, assert_bitwise, bits_equal
from forcing_layout_ref import layout_products

pytestmark = pytest.mark.gpu

SIG = evp.FIELDS[:12]
# the 11 layouts besides today's: (calc_strair, grid_ocn, grid_atm)
LAYOUTS = [(calc, ocn, atm) for ocn in "ABC" for calc, atm in ((True, "A"), (False, "A"), (False, "B"), (False, "C"))
           if (calc, ocn) != (True, "A")]
PPD = dict(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11, dyn_mass_min=1e-10)


def prep_params(c: GoldenCase):
    d = c.prep_scal_dict()
    return evp.PrepParams(dt=d["dt"], rhoi=d["rhoi"], rhos=d["rhos"], gravit=d["gravit"], dyn_area_min=d["dyn_area_min"],
                          dyn_mass_min=d["dyn_mass_min"], ssh_stress_coupled=d["ssh_coupled"])


def bgrid_core(c: GoldenCase):
    d, keep = c.hip_dims()
    core = evp.EvpHip(d, evp.make_params(c.scal_dict(), strict=True), c.d["HTE"], c.d["HTN"], c.d["dxT"], c.d["dyT"],
                      c.d["uarear"], c.d["tarea"], keepalive=keep, testing=True)
    if c.ns in ("tripole", "tripoleT"):
        core.set_metrics(dxhy=c.d["dxhy"], dyhx=c.d["dyhx"])
    st = c.prep_static()
    core.set_prep_geometry(st["tmask"], st["umask"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
    return core


def cgrid_core(c: GoldenCase):
    d, keep = c.hip_dims()
    ua = c.d["uarea"]
    uarear = np.where(ua > 0, 1.0 / np.where(ua > 0, ua, 1.0), 0.0)
    core = evp.EvpHip(d, evp.make_params(c.scal_dict(), strict=True), c.d["dyE"], c.d["dxN"], c.d["dxT"], c.d["dyT"], uarear,
                      c.d["tarea"], keepalive=keep, testing=True)
    core.cgrid_set_geometry(c.cgrid_static())
    core.cgrid_set_prep_geometry(c.cgrid_prep_static())
    return core


def physical(c: GoldenCase):
    m = np.zeros((c.nblocks, c.ny_block, c.nx_block), bool)
    for b in range(c.nblocks):
        ilo, ihi, jlo, jhi = (int(v) for v in c.blk[b, :4])
        m[b, jlo - 1:jhi, ilo - 1:ihi] = True
    return m


def bgrid_prep_and_loop(core, c, pp, icall, t, state, dyn):
    """cice_evp_hip_prep -> host strength -> loop; the products and the loop's outputs."""
    tm, um, _ = core.prep(pp, t, dict(state, TbU=dyn["TbU"]))
    out = {k: core.prep_fetch(k) for k in evp.PREP_FETCH}
    out.update(iceTmask=tm, iceUmask=um)
    raw = core.download()
    out.update({k: raw[k] for k in SIG})
    core.set_strength(dyn["strength"])
    core.subcycle(c.ndte)
    if c.ns in ("tripole", "tripoleT"):
        core.stress_halo()
    return out, core.download()


B_PINNED = [n for n in GOLDEN_CASES + TFOLD_CASES if GoldenCase(n).prep_scal_dict()["ssh_coupled"] == 0]


@pytest.mark.parametrize("name", B_PINNED)
def test_bgrid_layouts_reproduce_the_fixture(name):
    """B grid, every fixture with geostrophic tilt: the default run's uocnU, vocnU, strairxU, strairyU (ss_tltxU / yU) fed
    back as U-located uocn, vocn, strax, stray under ocean B / calc_strair = .false. / atmosphere B give the fixture's
    preparation products (the copied arrays on the physical cells: their ghost cells are the exchange's, not 0) and the
    fixture's loop outputs, bit for bit.  Then atmosphere A with strax = strairxT, its ghost cells filled by the centre
    vector exchange: every product and output equal to the fixture's.  (tripoleT: the centre rule rewrites the top row of an
    ocean field on any grid -- there the ocean stays on A.)"""
    from test_oracle_golden import check_prep_products
    c = GoldenCase(name)
    dom = c.oracle_domain()
    phys = physical(c)
    pp = prep_params(c)
    core = bgrid_core(c)
    try:
        for icall in range(1, c.ncalls + 1):
            t, state = c.prep_inputs(icall)
            dyn, _, _ = c.inputs(icall)
            core.set_forcing_layout(True, "A", "A")
            base, res = bgrid_prep_and_loop(core, c, pp, icall, t, state, dyn)
            assert_bitwise(res, c.expected(icall, c.ndte), f"{name} call {icall}: default layout")
            ss = {k: core.prep_fetch(k) for k in ("ss_tltxU", "ss_tltyU")}
            ocn = "A" if c.ns == "tripoleT" else "B"
            tu = dict(t, strax=base["strairxU"], stray=base["strairyU"])
            if ocn == "B":
                tu.update(uocn=base["uocnU"], vocn=base["vocnU"], ss_tltx=ss["ss_tltxU"], ss_tlty=ss["ss_tltyU"])
            core.set_forcing_layout(False, ocn, "B")
            out, res = bgrid_prep_and_loop(core, c, pp, icall, tu, state, dyn)
            for k in ("uocnU", "vocnU", "strairxU", "strairyU"):
                assert bits_equal(out[k][phys], base[k][phys]), f"{name} call {icall}: {k}"
                out[k] = np.where(phys, out[k], base[k])
            check_prep_products(c, icall, out, f"{name} call {icall} ocean {ocn}, strax / stray at U")
            assert_bitwise(res, c.expected(icall, c.ndte), f"{name} call {icall}: ocean {ocn}, atmosphere B")
            sx, sy = t["strairxT"].copy(), t["strairyT"].copy()
            oracle.halo_update(dom, sx, "center", "vector")
            oracle.halo_update(dom, sy, "center", "vector")
            core.set_forcing_layout(False, "A", "A")
            out, res = bgrid_prep_and_loop(core, c, pp, icall, dict(t, strax=sx, stray=sy), state, dyn)
            check_prep_products(c, icall, out, f"{name} call {icall} strax = strairxT")
            assert_bitwise(res, c.expected(icall, c.ndte), f"{name} call {icall}: calc_strair = .false., atmosphere A")
    finally:
        core.finalize()


def cgrid_finish_and_loop(core, c, icall):
    """The fixture's TbE / TbN (the reference's libm), its strength, then the loop: the 19 outputs."""
    _, want_in, _ = c.cgrid_inputs(icall)
    core.cgrid_set_tb(want_in["TbE"], want_in["TbN"])
    core.cgrid_prep_finish(c.d[f"in{icall:02d}_strength"], str(c.d["visc_method"]))
    nsub = c.nsub_list[-1]
    core.cgrid_subcycle(nsub)
    out = core.cgrid_download()
    dom = c.oracle_domain()
    oracle.halo_update(dom, out["strintxE"], "Eface", "vector")
    oracle.halo_update(dom, out["strintyN"], "Nface", "vector")
    return out, c.cgrid_expected(icall, nsub)


@pytest.mark.parametrize("name", CGRID_CASES + CGRID_TFOLD_CASES)
def test_cgrid_layouts_reproduce_the_fixture(name):
    """C grid, every fixture: calc_strair = .false. with strax = strairxT (ghost cells by the centre vector exchange) on
    atmosphere A, then atmosphere C with strax at E := strairxE and stray at N := strairyN as that run averaged them --
    the preparation's inputs of the loop and all 19 loop outputs equal the fixture's, bit for bit."""
    c = GoldenCase(name)
    dom = c.oracle_domain()
    pp = prep_params(c)
    core = cgrid_core(c)
    try:
        icall = 1
        t, st, _ = c.cgrid_prep_inputs(icall)
        state = {k: st[k] for k in oracle.C_FIELDS[:12]}
        prev = {k: st[k] for k in ("iceUmask", "iceEmask", "iceNmask")}
        _, want_in, want_masks = c.cgrid_inputs(icall)
        sx, sy = t["strairxT"].copy(), t["strairyT"].copy()
        oracle.halo_update(dom, sx, "center", "vector")
        oracle.halo_update(dom, sy, "center", "vector")
        keys = [k for k in evp.CGRID_INPUTS if k not in ("strength", "TbE", "TbN")]
        runs = []
        for atm in ("A", "C"):
            core.set_forcing_layout(False, "A", atm)
            tw = dict(t, strax=sx, stray=sy) if atm == "A" else dict(t, strax=runs[0]["strairxE"], stray=runs[0]["strairyN"])
            masks = core.cgrid_prep(pp, tw, state, prev)
            for k in oracle.C_MASKS:
                assert bits_equal(masks[k] != 0, want_masks[k] != 0), f"{name} atmosphere {atm}: {k}"
            got = {k: core.cgrid_fetch(k) for k in keys + evp.CGRID_FORCING_PRODUCTS[:2]}
            assert_bitwise({k: got[k] for k in keys}, {k: want_in[k] for k in keys}, f"{name} atmosphere {atm}: loop inputs")
            runs.append(got)
            out, want = cgrid_finish_and_loop(core, c, icall)
            assert_bitwise(out, want, f"{name} atmosphere {atm}: the loop from the device preparation")
        assert np.abs(runs[0]["strairxE"]).max() > 0
    finally:
        core.finalize()


# ---- every layout against the restatement: synthetic grids (closed, tripole u-fold) and a tripoleT fixture ----

def synth_case(grid, bs):
    spec = synth.GRIDS[grid]
    nx, ny, ns = spec["nx"], spec["ny"], spec.get("ns", "closed")
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=ns))
    cg = synth.cgrid_geometry(g)
    state, inputs, masks = synth.cgrid_state(g, cg, case="full", seed=9, warm=True)
    t, st7, prev = synth.cgrid_prep_inputs(g, cg, case="full", seed=17, coupled=True)
    dc = decomp.Decomp(nx, ny, *(bs or (nx, ny)), "cyclic", ns, 1)
    static, state, inputs, masks = synth.cgrid_scatter(dc, 0, cg, state, inputs, masks)
    vec = ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT")
    tb = {k: dc.scatter(v, 0, fold=("center", -1.0 if k in vec else 1.0)) for k, v in t.items()}
    loc = {"umaskCD": "NEcorner", "emask": "Eface", "nmask": "Nface", "fcor_blk": "NEcorner", "fcorE_blk": "Eface", "fcorN_blk": "Nface"}
    static.update({k: dc.scatter(v, 0, fill=0, fold=(loc.get(k, "center"), 1.0)) for k, v in st7.items()})
    prevb = {k: dc.scatter(v, 0, fill=0) for k, v in prev.items()}
    d, keep = evp.make_dims(dc, 0)
    blks = dc.local_blocks(0)
    dom = oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), dc.nx_global, dc.ny_global, dc.ew, dc.ns,
                              [b.ilo for b in blks], [b.ihi for b in blks], [b.jlo for b in blks],
                              [b.jhi for b in blks], [b.gi0 for b in blks], [b.gj0 for b in blks])
    blocks = [(b.ilo, b.ihi, b.jlo, b.jhi) for b in blks]
    mk = lambda: evp.EvpHip(d, evp.make_params(synth.evp_scalars(120), strict=True), static["dyE"], static["dxN"], static["dxT"],
                            static["dyT"], 1.0 / static["uarea"], static["tarea"], keepalive=keep, testing=True)
    return dict(mk=mk, dom=dom, blocks=blocks, static=static, t=tb, state={k: state[k] for k in evp.CGRID_FIELDS[:12]},
                prev=prevb, pp=evp.PrepParams(**PPD, ssh_stress_coupled=1), shape=dc.shape(0))


def fixture_case(name):
    c = GoldenCase(name)
    t, st, _ = c.cgrid_prep_inputs(1)
    static = c.cgrid_prep_static()
    ua = c.d["uarea"]
    uarear = np.where(ua > 0, 1.0 / np.where(ua > 0, ua, 1.0), 0.0)
    d, keep = c.hip_dims()
    mk = lambda: evp.EvpHip(d, evp.make_params(c.scal_dict(), strict=True), c.d["dyE"], c.d["dxN"], c.d["dxT"], c.d["dyT"],
                            uarear, c.d["tarea"], keepalive=keep, testing=True)
    return dict(mk=mk, dom=c.oracle_domain(), blocks=[tuple(int(v) for v in c.blk[b, :4]) for b in range(c.nblocks)],
                static=static, t=t, state={k: st[k] for k in oracle.C_FIELDS[:12]},
                prev={k: st[k] for k in ("iceUmask", "iceEmask", "iceNmask")}, pp=prep_params(c), shape=t["aice"].shape)


def located_inputs(S, seed):
    """Ocean fields and strax / stray for the layouts (values at whatever points the layout puts them; the preparation
    does not care where they came from): uocn, vocn, ss_tltx, ss_tlty as the device receives them and after the centre
    vector exchange (what the averages read), strax / stray with ghost cells that no exchange would give them."""
    f = synth.located_forcing(S["shape"], seed)
    t = dict(S["t"], uocn=f["uocn"], vocn=f["vocn"], ss_tltx=f["ss_tltx"], ss_tlty=f["ss_tlty"], strax=f["strax"], stray=f["stray"])
    ref = dict(t)
    for k in ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT"):
        ref[k] = np.ascontiguousarray(t[k], dtype=np.float64).copy()
        oracle.halo_update(S["dom"], ref[k], "center", "vector")
    return t, ref


CASES = [("gx3", None), ("gx3", (25, 29)), ("gx1", None), ("gx1", (80, 96)), ("tx1", None), ("tx1", (90, 60)),
         ("cgtript_cyc_1blk_full_avgstrength", None), ("cgtript_cyc_2x2_patchy", None)]


@pytest.mark.parametrize("grid_ice", ["B", "C"])
@pytest.mark.parametrize("case,bs", CASES)
def test_every_layout_against_the_restatement(case, bs, grid_ice):
    """The 11 layouts besides the default, on both grids: every averaged forcing product (uocnU, vocnU, ss_tltxU, ss_tltyU,
    strairxU, strairyU on the B grid; uocnE, vocnE, uocnN, vocnN and the ss_tltxE, ss_tltyN, strairxE, strairyN dyn_prep2
    reads on the C grid), every cell, against forcing_layout_ref applied to the same inputs, bit for bit."""
    S = fixture_case(case) if case in CGRID_TFOLD_CASES else synth_case(case, bs)
    st = S["static"]
    area = {"T": st["tarea"], "U": st["uarea"], "E": st["earea"], "N": st["narea"]}
    pm = {"T": st["hm"], "U": st["uvm"], "E": st["epm"], "N": st["npm"]}
    t, ref = located_inputs(S, seed=3)
    core = S["mk"]()
    try:
        if grid_ice == "B":
            core.set_prep_geometry(st["tmask"], st["umaskCD"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
            z = np.zeros(S["shape"])
            state = dict({k: z for k in SIG}, uvel=z, vvel=z, iceUmask=S["prev"]["iceUmask"])
        else:
            core.cgrid_set_geometry(st)
            core.cgrid_set_prep_geometry(st)
        nonzero = 0
        for calc, ocn, atm in LAYOUTS:
            core.set_forcing_layout(calc, ocn, atm, earea=st["earea"], narea=st["narea"], uvm=st["uvm"], epm=st["epm"], npm=st["npm"])
            want = layout_products(grid_ice, calc, ocn, atm, ref, area, pm, S["blocks"])
            if grid_ice == "B":
                core.prep(S["pp"], t, state)
                got = {k: core.prep_fetch(k) for k in want}
            else:
                core.cgrid_prep(S["pp"], t, S["state"], S["prev"])
                got = {k: core.cgrid_fetch(k) for k in want}
            assert_bitwise(got, want, f"{case} {bs} grid {grid_ice}: calc_strair {calc}, ocean {ocn}, atmosphere {atm}")
            nonzero += all(np.abs(w).max() > 0 for w in want.values())
            assert not np.array_equal(want[next(k for k in want if k.startswith("ss_tltx"))],
                                      want[next(k for k in want if k.startswith("ss_tlty"))])
        assert nonzero == len(LAYOUTS)
    finally:
        core.finalize()


def test_refusals_leave_the_layout_as_it_was():
    """An NE (grid 'CD') code and calc_strair = .false. without strax / stray are refused with a message; the default
    preparation right after still reproduces its fixture."""
    from test_oracle_golden import check_prep_products
    c = GoldenCase("pop_cyc_2x2_cap05")
    core = bgrid_core(c)
    try:
        with pytest.raises(evp.EvpHipError, match="NE"):
            core.set_forcing_layout(True, "CD", "A")
        with pytest.raises(evp.EvpHipError, match="NE"):
            core.set_forcing_layout(False, "A", (0, 4))
        with pytest.raises(evp.EvpHipError, match="0 T, 1 U"):
            core.set_forcing_layout(True, (0, 7), "A")
        t, state = c.prep_inputs(1)
        dyn, _, _ = c.inputs(1)
        core.set_forcing_layout(False, "A", "B")
        with pytest.raises(evp.EvpHipError, match="strax"):
            core.prep(prep_params(c), dict(t, strairxT=None, strairyT=None), dict(state, TbU=dyn["TbU"]))   # NULL wind slots
        core.set_forcing_layout(True, "A", "A")
        with pytest.raises(evp.EvpHipError, match="NE"):
            core.set_forcing_layout(False, "C", "CD")
        out, res = bgrid_prep_and_loop(core, c, prep_params(c), 1, t, state, dyn)
        check_prep_products(c, 1, out, "default layout after refusals")
        assert_bitwise(res, c.expected(1, c.ndte), "default layout after refusals")
        # a B-grid source on E points needs earea / epm
        core.set_forcing_layout(True, "C", "A")
        with pytest.raises(evp.EvpHipError, match="earea"):
            core.prep(prep_params(c), t, dict(state, TbU=dyn["TbU"]))
    finally:
        core.finalize()
