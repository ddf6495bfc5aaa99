"""GPU (-m gpu): the lean variant of the on-chip resident B-grid kernel (one rank, one block, no fold, TbU == 0, water ==
ocean current, revp == 0) against the general kernel on the same inputs, bit for bit (fp64 compared as uint64 patterns).
CICE_EVP_HIP_RES_LEAN=0 (test build) forces the general kernel where the lean one would run; every condition the lean
variant fixes has a case of its own that has to take the general kernel whatever the switch says."""
import numpy as np
import pytest

from cice_amd import evp, synth
from common import TFOLD_CASES, GoldenCase, assert_bitwise
from test_gpu_parity import synth_case

pytestmark = pytest.mark.gpu


def _run(monkeypatch, lean, dc, geo, fields, tm, um, scal, ndte):
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LOGW", "4")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LEAN", "1" if lean else "0")
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"],
                      geo["uarear"], geo["tarea"], keepalive=keep)
    try:
        out = core.run(fields, tm, um, ndte=ndte)
        tmg = core.timings()
        assert tmg["tile_variant"] == 2004, tmg
        assert tmg["resident_fallbacks"] == 0, tmg
        return out
    finally:
        core.finalize()


def _lean_vs_general(monkeypatch, grid, case, seed, ndte, scal=None, edit=None):
    dc, geo, fields, tm, um = synth_case(grid, case, seed=seed, warm=True)
    if edit:
        edit(fields, tm, um)
    scal = scal or synth.evp_scalars(120)
    general = _run(monkeypatch, False, dc, geo, fields, tm, um, scal, ndte)
    lean = _run(monkeypatch, True, dc, geo, fields, tm, um, scal, ndte)
    assert np.abs(general["uvel"]).max() > 1e-4          # the case moves ice
    assert_bitwise(lean, general, f"{grid}/{case}: lean vs general resident kernel")


@pytest.mark.parametrize("grid,case,ndte", [("gx3", "full", 120), ("gx3", "caps", 61), ("gx1", "full", 120), ("gx1", "caps", 33)])
def test_lean_resident_equals_general(grid, case, ndte, monkeypatch):
    """Even and odd subcycle counts: the lean loop takes two subcycles (one per record buffer) per trip."""
    _lean_vs_general(monkeypatch, grid, case, 20261016, ndte)


def _tbu_nonzero(fields, tm, um):
    fields["TbU"] = np.where(um != 0, 0.05 * fields["aiU"], 0.0)


def _water_not_ocean(fields, tm, um):
    fields["waterxU"] = fields["uocnU"] + 0.01
    fields["wateryU"] = fields["vocnU"] - 0.01


@pytest.mark.parametrize("what,edit,revised", [("TbU nonzero", _tbu_nonzero, False), ("water != ocean current", _water_not_ocean, False),
                                               ("revp", None, True)])
def test_lean_fallbacks_synthetic(what, edit, revised, monkeypatch):
    """Data the lean variant does not cover: the launch takes the general kernel with the switch on or off."""
    _lean_vs_general(monkeypatch, "gx3", "full", 7, 40, scal=synth.evp_scalars(120, revised_evp=revised), edit=edit)


@pytest.mark.skipif(not TFOLD_CASES, reason="no tripoleT fixture")
def test_lean_fallback_fold(monkeypatch):
    """A fold (tripoleT): the general kernel either way, and the reference's bits."""
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
    c = GoldenCase(TFOLD_CASES[0])
    outs = []
    for lean in ("1", "0"):
        monkeypatch.setenv("CICE_EVP_HIP_RES_LEAN", lean)
        d, keep = c.hip_dims()
        core = evp.EvpHip(d, evp.make_params(c.scal_dict(), strict=True), c.d["HTE"], c.d["HTN"], c.d["dxT"], c.d["dyT"],
                          c.d["uarear"], c.d["tarea"], keepalive=keep)
        core.set_metrics(dxhy=c.d["dxhy"], dyhx=c.d["dyhx"])
        try:
            dyn, tm, um = c.inputs(1)
            nsub = c.nsub_list[-1]
            outs.append(core.run(dyn, tm, um, ndte=nsub))
            assert core.timings()["tile_variant"] >= 2000
        finally:
            core.finalize()
    assert_bitwise(outs[0], outs[1], f"{c.ns}: lean switch on vs off")
    want = c.expected(1, nsub)
    assert_bitwise({k: outs[0][k] for k in ("uvel", "vvel")}, {k: want[k] for k in ("uvel", "vvel")}, f"{c.ns}: velocities vs reference")
