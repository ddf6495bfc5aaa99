"""GPU (-m gpu): the rim-wave schedule of the lean on-chip resident B-grid kernel (evp_resident2.hip, RIMU: the edge U-cells
in the wave that polls the ring, interior waves synchronised through three LDS slots, one workgroup barrier per subcycle) against
the oracle, the general kernel (CICE_EVP_HIP_RES_LEAN=0) and the lean loop's first schedule (CICE_EVP_HIP_RES_RIMU=0), all 18
outputs bit for bit (fp64 compared as uint64 patterns).  Every run asserts tile_variant == 2004 and resident_fallbacks == 0: a
protocol error shows as a failed test, not as a call repeated in silence; and describe_path says which schedule ran."""
import functools

import numpy as np
import pytest

from cice_amd import decomp, evp, synth
from common import assert_bitwise
from test_gpu_parity import run_oracle

pytestmark = pytest.mark.gpu

RIM, LEAN1, GENERAL = "rim", "lean", "general"
SWITCHES = {RIM: ("1", "1"), LEAN1: ("1", "0"), GENERAL: ("0", "1")}          # CICE_EVP_HIP_RES_LEAN, CICE_EVP_HIP_RES_RIMU
SCAL = synth.evp_scalars(120)


@functools.lru_cache(maxsize=None)
def _case(nx, ny, case, seed, holes=0.0):
    """One block, E-W cyclic, N-S closed; holes > 0: random, mutually independent T and U masks."""
    dx0 = synth.GRIDS["gx3"]["dx0"]
    g = synth.derive_geometry(synth.make_grid(nx, ny, dx0, ns="closed"))
    st = synth.make_state(g, case=case, seed=seed, warm=True)
    tmg, umg = st["iceTmask"], st["iceUmask"]
    if holes:
        rng = np.random.default_rng(seed)
        tmg = (tmg * (rng.random((ny, nx)) > holes)).astype(np.int32)
        umg = (umg * (rng.random((ny, nx)) > holes)).astype(np.int32)
        for k in evp.FIELDS[:12]:                      # dyn_prep2 zeroes the stresses off the ice
            st[k] = st[k] * tmg
        for k in ("uvel", "vvel", "uvel_init", "vvel_init"):
            st[k] = st[k] * umg
    dc = decomp.Decomp(nx, ny, nx, ny, "cyclic", "closed", 1)
    geo = {k: dc.scatter(g[k], 0, fill=(1.0 if k in ("HTE", "HTN", "dxT", "dyT", "tarea") else 0.0))
           for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
    fields = {k: dc.scatter(st[k], 0) for k in evp.FIELDS}
    return dc, geo, fields, dc.scatter(tmg, 0, fill=0), dc.scatter(umg, 0, fill=0)


@functools.lru_cache(maxsize=None)
def _oracle(key, ndte):
    return run_oracle(*_case(*key), SCAL, ndte)


def _run(monkeypatch, which, key, counts):
    """One EvpHip on the case, subcycle(n) for every n of counts on the one state."""
    lean, rimu = SWITCHES[which]
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LOGW", "4")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LEAN", lean)
    monkeypatch.setenv("CICE_EVP_HIP_RES_RIMU", rimu)
    dc, geo, fields, tm, um = _case(*key)
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
        assert tmg["tile_variant"] == 2004, tmg
        assert tmg["resident_fallbacks"] == 0, tmg
        assert ("edge U-cells in the rim wave" in core.describe_path()) == (which == RIM), core.describe_path()
        return out
    finally:
        core.finalize()


def _check(monkeypatch, key, counts):
    want = _oracle(key, sum(counts))
    assert np.abs(want["uvel"]).max() > 1e-4          # the case moves ice
    rim = _run(monkeypatch, RIM, key, counts)
    assert_bitwise(rim, want, f"{key} {counts}: rim-wave schedule vs oracle")
    assert_bitwise(rim, _run(monkeypatch, GENERAL, key, counts), f"{key} {counts}: rim-wave schedule vs general kernel")
    assert_bitwise(rim, _run(monkeypatch, LEAN1, key, counts), f"{key} {counts}: rim-wave schedule vs the lean loop's first schedule")


@pytest.mark.parametrize("ndte", [1, 2, 7, 61])
@pytest.mark.parametrize("case", ["full", "caps"])
def test_rim_schedule_gx3(case, ndte, monkeypatch):
    """Odd and even subcycle counts: the loop takes two subcycles (one per record buffer) per trip."""
    _check(monkeypatch, (100, 116, case, 20261018), (ndte,))


def test_rim_schedule_two_calls_on_one_state(monkeypatch):
    """7 then 8 subcycles: the record parity, the launch epoch and the slots' start carry over from call to call."""
    _check(monkeypatch, (100, 116, "full", 5), (7, 8))


@pytest.mark.parametrize("nx,ny", [(15, 15), (31, 16)])
def test_rim_schedule_small_cyclic_domains(nx, ny, monkeypatch):
    """One tile that polls its own images across the cyclic boundary; a last tile row with a single U-row."""
    _check(monkeypatch, (nx, ny, "full", 3), (9,))


@pytest.mark.parametrize("seed,holes", [(31, 0.35), (32, 0.7)])
def test_rim_schedule_random_independent_masks(seed, holes, monkeypatch):
    """Tiles with one, two or three ice-holding chunks, tiles that do not run, U-cells with ice among T-cells without."""
    _check(monkeypatch, (100, 116, "full", seed, holes), (9,))


def test_rim_schedule_survives_lagging_tiles(monkeypatch):
    """Every fourth tile delayed by 10 us per subcycle (CICE_EVP_HIP_RES_DEBUG=8): a slow neighbour must not let a wave read a
    plane or a velocity early."""
    monkeypatch.setenv("CICE_EVP_HIP_RES_DEBUG", "8")
    key = (100, 116, "full", 21)
    assert_bitwise(_run(monkeypatch, RIM, key, (24,)), _oracle(key, 24), "lagging tiles, rim-wave schedule vs oracle")
