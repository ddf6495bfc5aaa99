"""GPU (-m gpu): the lean resident B-grid loops on the range-proved square root and division (cice_amd/csrc/evp_range_math.h:
a wave whose active lanes all have their operands inside the window takes the cores, any other wave the compiler's forms)
against the oracle and against the same library with the switch off (CICE_EVP_HIP_RES_RANGE=0), all 18 outputs as uint64
patterns, on the rim-wave schedule and on the first lean loop (CICE_EVP_HIP_RES_RIMU=0).  States:
  a  ordinary
  b  velocities and ocean currents exactly zero on a patch that covers whole waves and parts of waves: Delta = 0 and
     du^2 + dv^2 = 0 there, the waves that hold such cells take the compiler's forms
  c  velocities scaled to about 1e-125 on the patch: Delta^2 < 2^-767, where the compiler's square root rescales
  d  strength = 0 on a patch of ice cells (a per-call operand outside the window: classified once, before the loop)
  e  one cell per 15 x 15 tile out of the window (strength, velocities and currents zero), the rest ordinary
  e2 the same on one cell in 35 all over, so that nearly every wave is mixed
  f  two calls on one state (ordinary)"""
import functools

import numpy as np
import pytest

from cice_amd import evp
from common import assert_bitwise
from test_gpu_parity import run_oracle
from test_gpu_resident_rim_u import SCAL, _case

pytestmark = pytest.mark.gpu

DOMAINS = {"15x15": (15, 15, "full", 3), "31x16": (31, 16, "full", 3),
           "gx3-full": (100, 116, "full", 20261018), "gx3-caps": (100, 116, "caps", 20261018)}
VEL = ("uvel", "vvel")
OCN = ("uocnU", "vocnU", "waterxU", "wateryU")


@functools.lru_cache(maxsize=None)
def _state(dom, which):
    """(dc, geo, fields, tm, um) of the domain with the state changed as the module's text says; arrays are (1, ny + 2, nx + 2)."""
    dc, geo, fields, tm, um = _case(*DOMAINS[dom])
    f = {k: np.array(v, copy=True) for k, v in fields.items()}
    ny, nx = f["uvel"].shape[-2] - 2, f["uvel"].shape[-1] - 2
    # a patch off the block's edge: a third of the rows and half of the columns, not aligned with tiles or waves
    j0, j1, i0, i1 = 3, 3 + max(5, ny // 3), 4, 4 + max(6, nx // 2)
    patch = np.zeros(f["uvel"].shape, bool)
    patch[:, j0:j1, i0:i1] = True
    sparse = np.zeros(f["uvel"].shape, bool)
    assert (np.asarray(tm)[patch] > 0).sum() > 64 or ny < 20, "the patch must hold ice cells"
    if which == "b":
        for k in VEL + OCN:
            f[k][patch] = 0.0
    elif which == "c":
        for k in VEL:
            f[k][patch] *= 1e-124
        assert 0 < np.abs(f["uvel"][patch]).max() < 1e-124
    elif which == "d":
        f["strength"][patch] = 0.0
    elif which in ("e", "e2"):
        if which == "e":
            sparse[:, 8:ny + 1:15, 8:nx + 1:15] = True      # tiles own 15 x 15 cells from the block's first cell on
        else:
            sparse[:, 2:ny:5, 2:nx:7] = True
        for k in VEL + OCN + ("strength",):
            f[k][sparse] = 0.0
    else:
        assert which in ("a", "f")
    for v in f.values():
        v.setflags(write=False)
    return dc, geo, f, tm, um


@functools.lru_cache(maxsize=None)
def _oracle(dom, which, ndte):
    return run_oracle(*_state(dom, which), SCAL, ndte)


def _run(monkeypatch, dom, which, counts, rimu, rng):
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LOGW", "4")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LEAN", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RES_RIMU", "1" if rimu else "0")
    monkeypatch.setenv("CICE_EVP_HIP_RES_RANGE", "1" if rng else "0")
    dc, geo, fields, tm, um = _state(dom, which)
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(SCAL, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"],
                      geo["uarear"], geo["tarea"], keepalive=keep)
    try:
        core.upload(fields, tm, um)
        for n in counts:
            core.subcycle(n)
        core.sync()
        out = core.download()
        tmg = core.timings()
        assert tmg["tile_variant"] == 2004, tmg          # the lean kernel ran ...
        assert tmg["resident_fallbacks"] == 0, tmg       # ... and no call was repeated on another path
        assert ("edge U-cells in the rim wave" in core.describe_path()) == rimu, core.describe_path()
        return out
    finally:
        core.finalize()


def _check(monkeypatch, dom, which, counts):
    want = _oracle(dom, which, sum(counts))
    assert len(want) == 18
    assert np.abs(want["uvel"]).max() > 1e-4          # the case moves ice
    for rimu in (True, False):
        name = "rim-wave schedule" if rimu else "first lean loop"
        got = _run(monkeypatch, dom, which, counts, rimu, True)
        assert_bitwise(got, want, f"{dom} {which} {counts}, {name}: range-proved arithmetic vs oracle")
        assert_bitwise(got, _run(monkeypatch, dom, which, counts, rimu, False), f"{dom} {which} {counts}, {name}: range-proved arithmetic vs switch off")


@pytest.mark.parametrize("ndte", [1, 2, 7])
@pytest.mark.parametrize("which", ["a", "b", "c", "d", "e", "e2"])
@pytest.mark.parametrize("dom", list(DOMAINS))
def test_range_math_states(dom, which, ndte, monkeypatch):
    _check(monkeypatch, dom, which, (ndte,))


@pytest.mark.parametrize("dom", list(DOMAINS))
def test_range_math_two_calls_on_one_state(dom, monkeypatch):
    _check(monkeypatch, dom, "f", (2, 7))
