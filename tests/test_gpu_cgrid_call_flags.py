"""GPU (-m gpu): the C grid's per-call verdict (evp_cgrid.hip: cg_call_setup -> CG.fast: waterx == uocn, Tb == +0, rheofact == 1
bit for bit on every ice face) with ONE deviating face (tests/call_flag_cases.py; tests/test_call_flags_cases_cpu.py shows that
every such face changes the oracle's bits), on every schedule that consumes it: the one-launch kernel cg_one, the fused
three-launch schedule, the five phase kernels, the marched kernel cg_strip and the on-chip resident kernel cg_res (fast or SLOW).
Each schedule is ONE core running default -> A -> default -> B -> A and B -> default: the captured graphs are keyed by the verdict.
Every call: all 19 arrays on every cell against the oracle as bit patterns, the flag word (a real deviation sets exactly its bit)
and CG.fast (taken whenever no bit is set, never otherwise)."""
import numpy as np
import pytest

import call_flag_cases as cf
from cice_amd import evp
from common import assert_bitwise
from evp_cgrid_call_chain import CG_PATHS, CG_SWITCHES as SWITCHES

pytestmark = pytest.mark.gpu

# the schedules and their switches: the rows of the one table of C-grid schedules that this file runs (tests/evp_cgrid_call_chain.py:
# CG_PATHS, as the B-grid file takes its rows from evp_call_chain.PATHS); schedule -> (environment, 3 x 3 padded blocks or one block)
PATHS = {p: (r.env, r.flags_split) for p, r in CG_PATHS.items() if r.flags_split is not None}


def make_core(monkeypatch, env, split):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    base = cf.c_base()
    static = cf.c_inputs(split, ())[0]
    d, keep = evp.make_dims(base.dcs[split], 0)
    core = evp.EvpHip(d, evp.make_params(cf.SCAL, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                      1.0 / static["uarea"], static["tarea"], keepalive=keep, testing=True)
    core.cgrid_set_geometry(static)
    return core


def check_path(core, path, what):
    t = core.cgrid_timings()
    n = cf.NDTE - 1                       # the first subcycle of a call runs as phases
    assert t["resident_fallbacks"] == 0, (what, t)
    if path == "cg_one":
        assert t["one_launch_subcycles"] == n and t["marched_items"] == 0 and t["resident_subcycles"] == 0, (what, t)
    elif path == "cg_strip":
        assert t["one_launch_subcycles"] == n and t["marched_items"] > 0 and t["resident_subcycles"] == 0, (what, t)
    elif path.startswith("cg_res"):
        assert t["resident_subcycles"] == n, (what, t)
    else:
        assert t["one_launch_subcycles"] == 0 and t["resident_subcycles"] == 0, (what, t)


def run_and_check(core, path, split, devs, what):
    _, state, inputs, masks = cf.c_inputs(split, devs)
    got = core.cgrid_run(cf.NDTE, state, inputs, masks)
    fl = core.call_flags()
    print(f"{what}: flag word {fl['cgrid']:#x}, fast {fl['cgrid_fast']}")
    assert_bitwise(got, cf.c_oracle(split, devs), what)
    check_path(core, path, what)
    return fl


@pytest.mark.parametrize("path", list(PATHS))
def test_one_face_deviations_in_a_sequence_of_calls(path, monkeypatch):
    env, split = PATHS[path]
    core = make_core(monkeypatch, env, split)
    try:
        for a, b in cf.c_pairs():
            for devs in ((), (a,), (), (b,), (a, b), ()):
                what = f"{path}: {devs or 'default'}"
                fl = run_and_check(core, path, split, devs, what)
                assert fl["cgrid"] & 7 == cf.c_bits(devs), (what, fl)           # exactly its bit
                assert fl["cgrid_fast"] == (cf.c_bits(devs) == 0), (what, fl)   # the shortcut taken whenever it may be, never otherwise
    finally:
        core.finalize()


@pytest.mark.parametrize("path", list(PATHS))
def test_null_deviations(path, monkeypatch):
    """The same values where the loop never reads them: a face without ice leaves the word clear and the shortcut taken; a ghost
    cell and a padding cell beyond ihi: only the bits are asserted, the read-out is printed."""
    env, split = PATHS[path]
    core = make_core(monkeypatch, env, split)
    try:
        for where in cf.C_NULLS if split else cf.C_NULLS[:1]:
            devs = tuple((k, where) for k in cf.C_KINDS)
            fl = run_and_check(core, path, split, devs, f"{path}: null deviations at the {where}")
            if where == "interior cell without ice":
                assert fl["cgrid"] & 7 == 0 and fl["cgrid_fast"], fl
    finally:
        core.finalize()


@pytest.mark.parametrize("path", list(PATHS))
def test_shortcut_switched_off_gives_the_same_bits(path, monkeypatch):
    """A/B: CICE_EVP_HIP_CGRID_FAST=0 keeps the default-configuration kernels from ever being taken; the default state and a
    deviation of every kind give the oracle's bits again, and the read-out says the shortcut was not taken."""
    env, split = PATHS[path]
    core = make_core(monkeypatch, dict(env, CICE_EVP_HIP_CGRID_FAST="0"), split)
    try:
        for devs in [()] + [((k, "last cell of the padded block"),) for k in cf.C_KINDS]:
            fl = run_and_check(core, path, split, devs, f"{path}, shortcut off: {devs or 'default'}")
            assert not fl["cgrid_fast"] and fl["cgrid"] & 7 == cf.c_bits(devs), fl
    finally:
        core.finalize()


def test_device_preparation_one_shallow_cell(monkeypatch):
    """The C grid's preparation on the device (cice_evp_hip_cgrid_prep, the seabed stress factors by LKD on the device,
    cice_evp_hip_cgrid_prep_finish) at gx3 size: deep water everywhere leaves the word clear and the shortcut taken; water shallow
    under exactly ONE T-cell gives TbE / TbN != 0 on at most two faces each and sets exactly the seabed bit -- the factors within
    2 ulp of the oracle's, zero pattern bit-equal, and the loop, fed by the oracle's preparation and those factors, equal to the
    oracle's bit for bit."""
    import oracle
    from common import bits_equal
    from test_gpu_seabed import ALPHAB, K1, K2, PPD, THR, cgrid_case
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_FAST", "1")               # (the test build, for the read-out; the shortcut allowed)
    core, dc, dom, scal, static, state, prevb, tb, want, inputs = cgrid_case("gx3", (30, 40))
    try:
        em, nm = want["iceEmask"] != 0, want["iceNmask"] != 0
        inner = np.zeros(em.shape, bool)
        inner[:, 3:-3, 3:-3] = True
        cells = np.argwhere(inner & em & nm & np.roll(em, 1, axis=2) & np.roll(nm, 1, axis=1) & (tb["vice"] > 1.0))
        assert len(cells) > 0
        cell = tuple(cells[len(cells) // 2])
        deep = np.full(em.shape, 80.0)
        shallow = deep.copy()
        shallow[cell] = 3.0
        prm = cf.oracle_params()
        for name, hw in (("deep", deep), ("shallow", shallow), ("deep again", deep)):
            got = core.cgrid_prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), tb, state, prevb)
            for k in ("iceTmask", "iceUmask", "iceEmask", "iceNmask"):
                assert bits_equal(got[k] != 0, want[k] != 0), k
            core.cgrid_seabed_lkd(hw, K1, K2, ALPHAB, THR)
            core.cgrid_prep_finish(inputs["strength"])
            fl = core.call_flags()
            tbs = {}
            for loc in "EN":
                w = oracle.seabed_lkd_c(dom, loc, K1, K2, ALPHAB, THR, tb["aice"], tb["vice"], hw, want[f"ice{loc}mask"])
                dev = core.cgrid_fetch("Tb" + loc)
                assert bits_equal(dev == 0, w == 0), (name, loc)
                nz = w != 0
                if name == "shallow":
                    assert 1 <= nz.sum() <= 2, (loc, int(nz.sum()))
                    assert (np.abs(dev[nz] - w[nz]) / np.spacing(np.abs(w[nz]))).max() <= 2.0
                else:
                    assert nz.sum() == 0
                tbs["Tb" + loc] = dev
            print(f"{name}: flag word {fl['cgrid']:#x}, fast {fl['cgrid_fast']}")
            assert fl["cgrid"] & 7 == (evp.CG_TB_NONZERO if name == "shallow" else 0) and fl["cgrid_fast"] == (name != "shallow"), fl
            core.cgrid_subcycle(cf.NDTE)
            win = {k: want[k] for k in oracle.C_INPUTS}
            win.update(tbs, strength=inputs["strength"])
            loop = oracle.cgrid_subcycle(dom, prm, cf.NDTE, {k: want[k] for k in oracle.C_FIELDS[:14]}, win, static,
                                         {k: want[k] for k in oracle.C_MASKS}, visc_method="avg_zeta")
            assert_bitwise(core.cgrid_download(), loop, f"C grid: device preparation + loop, {name}")
            assert core.cgrid_timings()["resident_fallbacks"] == 0
    finally:
        core.finalize()
