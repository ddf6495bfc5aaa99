"""GPU (-m gpu): the B grid's per-call and per-init shortcut verdicts -- EVP_F_WATER_IS_OCN, EVP_F_TBU_ZERO (host scan of
cice_evp_hip_upload, cice_evp_hip_set_tbu) and EVP_F_METRICS (cice_evp_hip_init, cice_evp_hip_set_metrics) -- with ONE deviating
cell (tests/call_flag_cases.py; tests/test_call_flags_cases_cpu.py shows that every such cell changes the oracle's bits), on every
kernel that consumes them: the streaming kernel, the on-chip resident kernel (general, and where the lean variant is eligible), the
marching kernel at four and two subcycles per pass.  Each path is ONE core running default -> A -> default -> B -> A and B ->
default, so that the transitions are covered: the lean kernel alternating with the general one, the marching host starting to pack
operands it did not pack before.  Every call: all 18 outputs on every cell against the oracle as bit patterns, the read-out of the
flags (a real deviation clears exactly its flag), and the evidence that the fast path ran whenever the flags allow it."""
import numpy as np
import pytest

import call_flag_cases as cf
import oracle
from cice_amd import evp
from common import assert_bitwise
from evp_call_chain import PATH_ENV, PATHS as PATH_SWITCHES

pytestmark = pytest.mark.gpu

OCN, TBU, MET, DXHY = evp.F_WATER_IS_OCN, evp.F_TBU_ZERO, evp.F_METRICS, evp.F_DXHY_ARRAY
# path -> (environment, 3 x 3 padded blocks or one block); the switches of a path are tests/evp_call_chain.py's, as is the list of
# switches cleared before a row's own are set
PATHS = {
    "streaming": (PATH_SWITCHES["streaming"], True),
    "resident general": (PATH_SWITCHES["resident general"], True),
    "resident lean-eligible": (PATH_SWITCHES["resident lean-eligible"], False),
    "marching k=4": (PATH_SWITCHES["marching k=4"], True),
    "marching k=2": (dict(PATH_SWITCHES["marching k=4"], CICE_EVP_HIP_MARCH_K="2"), False),
}


def make_core(monkeypatch, env, split, geo=None):
    for k in PATH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    base = cf.b_base()
    geo = geo or base.geo[split]
    d, keep = evp.make_dims(base.dcs[split], 0)
    return evp.EvpHip(d, evp.make_params(cf.SCAL, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"],
                      geo["tarea"], keepalive=keep, testing=True)


def check_path(core, path, shortcuts_hold, what):
    """The kernel the path names ran; where both per-call flags are set, in its fast form."""
    t, fl, m = core.timings(), core.call_flags(), core.march_info()
    assert t["resident_fallbacks"] == 0, (what, t)
    if path == "streaming":
        assert t["tile_variant"] < 1000 and not m["last_call"], (what, t, m)
    elif path == "resident general":
        assert t["tile_variant"] >= 2000 and not fl["resident_lean"], (what, t, fl)
    elif path == "resident lean-eligible":
        assert t["tile_variant"] == 2004 and fl["resident_lean"] == shortcuts_hold, (what, t, fl)
    else:
        assert m["mode"] == 1 and m["last_call"] and m["declined"] == 0 and m["kpass"] == int(path[-1]), (what, m)


def run_and_check(core, path, split, devs, flags0, what):
    fields, tm, um = cf.b_inputs(split, devs)
    got = core.run(fields, tm, um, ndte=cf.NDTE)
    fl = core.call_flags()["bgrid"]
    print(f"{what}: flags {fl:#x}")
    assert_bitwise(got, cf.b_oracle(split, devs), what)
    return fl


@pytest.mark.parametrize("path", list(PATHS))
def test_one_cell_deviations_in_a_sequence_of_calls(path, monkeypatch):
    env, split = PATHS[path]
    core = make_core(monkeypatch, env, split)
    try:
        flags0 = None
        for a, b in cf.b_pairs():
            for devs in ((), (a,), (), (b,), (a, b), ()):
                what = f"{path}: {devs or 'default'}"
                fl = run_and_check(core, path, split, devs, flags0, what)
                if flags0 is None:
                    flags0 = fl
                    assert flags0 & OCN and flags0 & TBU and flags0 & MET and not flags0 & DXHY, hex(flags0)
                # a real deviation clears exactly its flag and no other
                assert fl == flags0 & ~cf.b_cleared(devs), (what, hex(fl), hex(flags0))
                check_path(core, path, not cf.b_cleared(devs), what)
    finally:
        core.finalize()


@pytest.mark.parametrize("path", list(PATHS))
def test_null_deviations(path, monkeypatch):
    """The same values where the loop never reads them: an interior cell without ice, a ghost cell whose iceUmask is set (the image
    of an ice cell across the cyclic boundary) and a padding cell beyond ihi of a padded block.  The bits are the undeviated
    oracle's, every flag stays set and the fast path is taken: the host scan of cice_evp_hip_upload follows the blocks' rectangles,
    as the device scans of the preparation do.  The read-out is printed."""
    env, split = PATHS[path]
    core = make_core(monkeypatch, env, split)
    try:
        flags0 = run_and_check(core, path, split, (), None, f"{path}: default")
        for where in cf.B_NULLS if split else cf.B_NULLS[:1]:
            devs = tuple((k, where) for k in cf.B_KINDS)
            fl = run_and_check(core, path, split, devs, flags0, f"{path}: null deviations at the {where}")
            assert fl == flags0, (where, hex(fl), hex(flags0))
            check_path(core, path, True, where)
    finally:
        core.finalize()


@pytest.mark.parametrize("path", ["streaming", "resident general", "resident lean-eligible", "marching k=4"])
@pytest.mark.parametrize("bit", [TBU, OCN])
def test_masking_the_flag_off_gives_the_same_bits(path, bit, monkeypatch):
    """A/B: with CICE_EVP_HIP_FLAGS keeping the flag from ever being used, every real deviation of that flag gives the oracle's
    bits again -- the same bits as the run that dropped the flag by itself."""
    env, split = PATHS[path]
    core = make_core(monkeypatch, dict(env, CICE_EVP_HIP_FLAGS=hex(0xFFFFFFFF & ~bit)), split)
    try:
        for kind, where in cf.B_REAL:
            if cf.B_KINDS[kind][2] != bit:
                continue
            fl = run_and_check(core, path, split, ((kind, where),), None, f"{path}, flag {bit} masked off: {kind} at {where}")
            assert not fl & bit
        fl = run_and_check(core, path, split, (), None, f"{path}, flag {bit} masked off: default")
        assert not fl & bit and fl & (TBU | OCN)
        check_path(core, path, False, f"{path} masked")
    finally:
        core.finalize()


@pytest.mark.parametrize("path", ["streaming", "resident general", "marching k=4"])
def test_set_tbu_one_cell(path, monkeypatch):
    """cice_evp_hip_set_tbu re-derives TBU_ZERO on its own: upload the default state, then hand over a TbU with one cell 0.7, with one
    cell -0.0, and all zero again."""
    env, split = PATHS[path]
    core = make_core(monkeypatch, env, split)
    try:
        fields, tm, um = cf.b_inputs(split, ())
        for kind in ("TbU=0.7", "TbU=-0.0", None, "TbU=-0.0"):
            devs = ((kind, "last cell of the padded block"),) if kind else ()
            core.upload(fields, tm, um)
            flags0 = core.call_flags()["bgrid"]
            assert flags0 & TBU
            core.set_tbu(cf.b_inputs(split, devs)[0]["TbU"])
            fl = core.call_flags()["bgrid"]
            assert fl == (flags0 & ~TBU if kind else flags0), (kind, hex(fl))
            core.subcycle(cf.NDTE)
            assert_bitwise(core.download(), cf.b_oracle(split, devs), f"{path}: set_tbu with {kind}")
            check_path(core, path, not kind, f"{path}: set_tbu with {kind}")
    finally:
        core.finalize()


def oracle_with_static(split, geo, override=None):
    """The oracle on the default state with the metric terms of `geo` (oracle.metrics), some of them replaced."""
    base = cf.b_base()
    dc = base.dcs[split]
    blks = dc.local_blocks(0)
    dom = oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), dc.nx_global, dc.ny_global, dc.ew, dc.ns,
                              [b.ilo for b in blks], [b.ihi for b in blks], [b.jlo for b in blks], [b.jhi for b in blks],
                              [b.gi0 for b in blks], [b.gj0 for b in blks])
    m = oracle.metrics(dom, cf.SCAL["deltaminEVP"], geo["HTE"], geo["HTN"], geo["tarea"])
    static = dict(m, dxT=geo["dxT"], dyT=geo["dyT"], uarear=geo["uarear"])
    static.update(override or {})
    prm = oracle.make_params(**{k: cf.SCAL[k] for k in ("arlx1i", "denom1", "brlx", "revp", "e_factor", "epp2i", "capping", "Ktens",
                                                        "deltaminEVP", "u0", "cosw", "sinw", "rhow")})
    fields, tm, um = cf.b_inputs(split, ())
    out = oracle.subcycle(dom, prm, cf.NDTE, fields, static, tm, um)
    return m, {k: out[k] for k in evp.OUTPUTS}


def block_cell(split, p):
    """(block, row, column) in the block arrays of global cell p."""
    dc = cf.b_base().dcs[split]
    b = next(b for b in dc.blocks if b.gj0 - 1 <= p[0] < b.gj0 - 1 + b.gny and b.gi0 - 1 <= p[1] < b.gi0 - 1 + b.gnx)
    return b.local, p[0] - (b.gj0 - 1) + 1, p[1] - (b.gi0 - 1) + 1


@pytest.mark.parametrize("where", ["first cell of block 0", "last cell of the padded block", "alone in its tile"])
def test_tarea_one_ulp_off_clears_the_init_time_flag(where, monkeypatch):
    """tarea one ulp off dxT * dyT in ONE cell: the kernels may not derive DminTarea, EVP_F_METRICS is cleared at init; the
    streaming and resident kernels give the oracle's bits with oracle.metrics of that tarea, the marching path declines."""
    base = cf.b_base()
    split = True
    cell = block_cell(split, base.positions("TbU=0.7")[where])
    geo = {k: v.copy() for k, v in base.geo[split].items()}
    geo["tarea"][cell] = np.nextafter(geo["tarea"][cell], np.inf)
    _, want = oracle_with_static(split, geo)
    for path in ("streaming", "resident general", "marching k=4"):
        core = make_core(monkeypatch, PATHS[path][0], split, geo=geo)
        try:
            fields, tm, um = cf.b_inputs(split, ())
            got = core.run(fields, tm, um, ndte=cf.NDTE)
            fl = core.call_flags()["bgrid"]
            assert not fl & MET and fl & OCN and fl & TBU, hex(fl)
            assert_bitwise(got, want, f"{path}: tarea one ulp off at the {where}")
            if path.startswith("marching"):
                m = core.march_info()
                assert m["mode"] == 0 and not m["last_call"], m
                assert "metric terms come from arrays" in core.describe_path(), core.describe_path()
            else:
                check_path(core, path, True, path)
        finally:
            core.finalize()


@pytest.mark.parametrize("name", ["cxp", "dxhy", "DminTarea"])
def test_set_metrics_with_one_cell_nudged_is_honoured(name, monkeypatch):
    """cice_evp_hip_set_metrics with an array one ulp off the derived term in one ice T-cell: the kernels read the arrays from
    then on (dxhy: EVP_F_DXHY_ARRAY; the others: EVP_F_METRICS cleared) and give the oracle's bits with that static array -- which
    differ from the bits with the derived terms --; the marching path declines.  Arrays equal to the derived terms change nothing."""
    base = cf.b_base()
    split = True
    geo = base.geo[split]
    m, want0 = oracle_with_static(split, geo)
    assert not cf.differing(want0, cf.b_oracle(split, ()))
    # the cell: an ice T-cell of the padded last block, from its last physical cell backwards, the first where that ulp changes
    # the oracle's bits (DminTarea only matters where the ice is nearly at rest -- nowhere in this state: there the flags alone show the fix)
    b8 = base.dcs[split].blocks[8].local
    tm = cf.b_inputs(split, ())[1]
    want = None
    # (one ulp of dxhy shows at about one cell in 300: there the search runs over every block, from the first cell on)
    inner = np.zeros(tm.shape, bool)
    inner[:, 1:-1, 1:-1] = True
    cells = np.argwhere((tm != 0) & inner)
    cells = cells if name == "dxhy" else cells[cells[:, 0] == b8][::-1][:40]
    for cell in map(tuple, cells):
        arr = m[name].copy()
        arr[cell] = np.nextafter(arr[cell], np.inf)
        _, want = oracle_with_static(split, geo, {name: arr})
        if name == "DminTarea" or cf.differing(want, want0):
            break
    else:
        raise AssertionError(f"no ice T-cell where one ulp of {name} changes the oracle's outputs")
    for path in ("streaming", "resident general", "marching k=4"):
        core = make_core(monkeypatch, PATHS[path][0], split)
        try:
            flags0 = core.call_flags()["bgrid"]
            core.set_metrics(**m)                               # the derived terms themselves: nothing changes
            assert core.call_flags()["bgrid"] == flags0 and flags0 & MET and not flags0 & DXHY
            core.set_metrics(**{name: arr})
            fl = core.call_flags()["bgrid"]
            assert fl == (flags0 | DXHY if name == "dxhy" else flags0 & ~MET), (name, hex(fl), hex(flags0))
            fields, tm, um = cf.b_inputs(split, ())
            got = core.run(fields, tm, um, ndte=cf.NDTE)
            assert_bitwise(got, want, f"{path}: set_metrics({name} one ulp off in one cell)")
            if path.startswith("marching"):
                assert core.march_info()["mode"] == 0 and "metric terms come from arrays" in core.describe_path(), core.describe_path()
            else:
                check_path(core, path, True, path)
        finally:
            core.finalize()


def test_device_preparation_one_shallow_cell(monkeypatch):
    """The device scans (f-2): cice_evp_hip_prep, then the seabed stress factor by LKD on the device, on the gx3-sized state of
    test_prep_on_device_full_size_vs_oracle.  Deep water everywhere leaves TBU_ZERO set; water shallow under exactly ONE T-cell
    gives TbU != 0 on at most four U-cells and clears it -- TbU within 2 ulp of the oracle's (the device exp()), the zero pattern
    bit-equal, and the loop, fed by the oracle's preparation and that TbU, equal to the oracle's bit for bit."""
    from cice_amd import decomp, synth
    from common import bits_equal
    from test_gpu_seabed import ALPHAB, K1, K2, PPD, THR, oracle_domain
    monkeypatch.setenv("CICE_EVP_HIP_FLAGS", "0xffffffff")           # (the test build, for the read-out; every flag allowed)
    spec = synth.GRIDS["gx3"]
    nx, ny = spec["nx"], spec["ny"]
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns="closed"))
    pr = synth.make_primary(g, "full", seed=4)
    dc = decomp.Decomp(nx, ny, 25, 29, "cyclic", "closed", 1)
    sc = lambda a, fill=0.0: dc.scatter(np.ascontiguousarray(a), 0, fill=fill)
    geo = {k: sc(g[k], 1.0 if k != "uarear" else 0.0) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
    static = {k: sc(v, (1.0 if k in ("tarea", "uarea") else 0)) for k, v in pr["static"].items()}
    t = {k: sc(v) for k, v in pr["t"].items()}
    state = {k: sc(v) for k, v in pr["state"].items()}
    dom = oracle_domain(dc)
    z = np.zeros(dc.shape(0))
    want = oracle.prep(dom, oracle.PrepParams(**PPD, cosw=cf.SCAL["cosw"], sinw=cf.SCAL["sinw"], ssh_coupled=0), static, t,
                       dict(state, strintxU=z, strintyU=z, strocnxU=z, strocnyU=z))
    tm, um = want["iceTmask"], want["iceUmask"]
    strength = np.where(tm != 0, 2.75e4 * t["vice"] * np.exp(-20.0 * (1.0 - t["aice"])), 0.0)
    aice, vice = [oracle.halo_update(dom, np.array(t[k], dtype=np.float64, order="C", copy=True), "center", "scalar") for k in ("aice", "vice")]
    # the one shallow T-cell: inside a block (no ghost image), all four U-cells around it with ice and the ice thick enough to ground
    deep = np.full(dc.shape(0), 80.0)
    inner = np.zeros(um.shape, bool)
    inner[:, 3:-3, 3:-3] = True
    four = (um != 0) & np.roll(um != 0, 1, axis=1) & np.roll(um != 0, 1, axis=2) & np.roll(np.roll(um != 0, 1, axis=1), 1, axis=2)
    cells = np.argwhere(inner & four & (vice > 1.0))
    assert len(cells) > 0
    cell = tuple(cells[len(cells) // 2])
    shallow = deep.copy()
    shallow[cell] = 3.0
    m = oracle.metrics(dom, cf.SCAL["deltaminEVP"], geo["HTE"], geo["HTN"], geo["tarea"])
    ostatic = dict(m, dxT=geo["dxT"], dyT=geo["dyT"], uarear=geo["uarear"])
    prm = cf.oracle_params()
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(cf.SCAL, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"],
                      geo["tarea"], keepalive=keep)
    try:
        core.set_prep_geometry(static["tmask"], static["umask"], static["hm"], static["tarea"], static["uarea"], static["fcor_blk"])
        for name, hw in (("deep", deep), ("shallow", shallow), ("deep again", deep)):
            gtm, gum, _ = core.prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), t, state)
            assert bits_equal(gtm, tm) and bits_equal(gum, um)
            fl = core.call_flags()["bgrid"]
            assert fl & TBU and fl & OCN, hex(fl)                    # TbU not handed in: zero; cosw = 1, sinw = 0: water is the ocean current
            core.seabed_lkd(hw, K1, K2, ALPHAB, THR)
            fl = core.call_flags()["bgrid"]
            tb = core.prep_fetch("TbU")
            wtb = oracle.seabed_lkd(dom, K1, K2, ALPHAB, THR, aice, vice, hw, um)
            assert bits_equal(tb == 0, wtb == 0), name
            nz = wtb != 0
            print(f"{name}: flags {fl:#x}, TbU != 0 on {int(nz.sum())} U-cells")
            if name == "shallow":
                assert 1 <= nz.sum() <= 4 and not fl & TBU and fl & OCN, (int(nz.sum()), hex(fl))
                assert (np.abs(tb[nz] - wtb[nz]) / np.spacing(np.abs(wtb[nz]))).max() <= 2.0
            else:
                assert nz.sum() == 0 and fl & TBU and fl & OCN, (int(nz.sum()), hex(fl))
            core.set_strength(strength)
            core.subcycle(cf.NDTE)
            got = core.download()
            dyn = {k: want[k] for k in evp.FIELDS if k in want}
            dyn.update(strength=strength, TbU=tb, strintxU=z, strintyU=z, taubxU=z, taubyU=z)
            loop = oracle.subcycle(dom, prm, cf.NDTE, dyn, ostatic, tm, um)
            assert_bitwise(got, {k: loop[k] for k in evp.OUTPUTS}, f"device preparation + loop, {name}")
            if name == "shallow":
                assert np.abs(loop["taubxU"][nz]).max() > 0
            assert core.timings()["resident_fallbacks"] == 0
    finally:
        core.finalize()
