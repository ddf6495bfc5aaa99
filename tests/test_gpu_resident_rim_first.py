"""GPU (-m gpu): the three speed switches of the rim-wave schedule of the lean on-chip resident B-grid kernel (evp_resident2.hip,
subcycle_rim and the prologue above it):
  issue priorities (CICE_EVP_HIP_RES_PRIO = 0..3: none / the rim wave first while it is on the hand-off chain / and the interior
    waves' stress update raised / and all their arithmetic raised);
  full tiles taking the identity chunk map without the per-CU lock (CICE_EVP_HIP_RES_NOLOCK);
  the U-cells' two divisions on the range-proved cores, their reciprocal formed in the first part of the momentum step
    (CICE_EVP_HIP_RES_SPLITDIV; evp_range_math.h: recip_core / quot_core)
against the oracle and against the schedule with all three off, all 18 outputs bit for bit (fp64 compared as uint64 patterns).
None may change a bit: a priority only orders issue, any chunk -> wave map is correct, and the split division performs div_core's
operations on div_core's values.  (div_core IS quot_core(n, d, recip_core(d)): tests/test_gpu_range_math.py's sweep of div_core
against n / d -- window edges, exact and near-half-way quotients, both signs -- is the sweep of the split form; no second probe.)
Every run asserts tile_variant == 2004 and resident_fallbacks == 0: a starved wait gives up, and that shows as a failed test, not
as a call repeated in silence."""
import functools

import numpy as np
import pytest

from common import assert_bitwise
from test_gpu_parity import run_oracle
from test_gpu_resident_rim_u import SCAL, _case, _oracle
from test_gpu_resident_range_math import _oracle as _state_oracle, _state
from cice_amd import evp

pytestmark = pytest.mark.gpu

OFF = (0, 0, 0)                                # (priority form, full tiles skip the lock, split division): the schedule as it was
SINGLY = [(1, 0, 0), (2, 0, 0), (3, 0, 0), (0, 1, 0), (0, 0, 1)]
ALL_ON = [(1, 1, 1), (2, 1, 1), (3, 1, 1)]


def _run(monkeypatch, switches, case, counts, debug=None, stamps=False):
    """One EvpHip (test build) on the case (dc, geo, fields, tm, um) with the switches set, subcycle(n) for every n of counts on
    the one state.  stamps: with the phase stamps on, returns (outputs, passes on the compiler's sqrt / division per wave)."""
    prio, nolock, split = switches
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LOGW", "4")
    monkeypatch.setenv("CICE_EVP_HIP_RES_PRIO", str(prio))
    monkeypatch.setenv("CICE_EVP_HIP_RES_NOLOCK", str(nolock))
    monkeypatch.setenv("CICE_EVP_HIP_RES_SPLITDIV", str(split))
    if debug is not None:
        monkeypatch.setenv("CICE_EVP_HIP_RES_DEBUG", str(debug))
    if stamps:
        monkeypatch.setenv("CICE_EVP_HIP_RES_PROF", "1")
    dc, geo, fields, tm, um = case
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
        assert "edge U-cells in the rim wave" in core.describe_path(), core.describe_path()
        if stamps:
            return out, (core.debug_prof()[:, :, 6] >> np.uint64(8)).astype(np.int64)
        return out
    finally:
        core.finalize()


def _check(monkeypatch, key, counts, forms):
    want = _oracle(key, sum(counts))
    assert np.abs(want["uvel"]).max() > 1e-4          # the case moves ice
    off = _run(monkeypatch, OFF, _case(*key), counts)
    assert_bitwise(off, want, f"{key} {counts}: all switches off vs oracle")
    for sw in forms:
        assert_bitwise(_run(monkeypatch, sw, _case(*key), counts), off,
                       f"{key} {counts}: priorities {sw[0]}, lock skipped {sw[1]}, split division {sw[2]} vs all off")


@pytest.mark.parametrize("ndte", [1, 2, 7])
@pytest.mark.parametrize("case", ["full", "caps"])
def test_each_switch_singly_and_all_on(case, ndte, monkeypatch):
    """Odd and even trip counts of the two-subcycle loop; every switch alone, and all three."""
    _check(monkeypatch, (100, 116, case, 20261018), (ndte,), SINGLY + ALL_ON)


def test_two_calls_on_one_state(monkeypatch):
    """7 then 8 subcycles: a full tile that skipped the lock leaves no launch stamp behind, the partial tiles of the second call
    must still find a stale one and reset the per-CU counts; the rim wave's reciprocal of the first call's last subcycle is not
    the second call's."""
    _check(monkeypatch, (100, 116, "caps", 5), (7, 8), [(0, 1, 0), (0, 0, 1), (3, 1, 1)])


@pytest.mark.parametrize("nx,ny", [(15, 15), (31, 16)])
def test_small_cyclic_domains(nx, ny, monkeypatch):
    """One tile that polls its own images across the cyclic boundary (its raised rim wave waits for records it stores itself);
    a last tile row with a single U-row."""
    _check(monkeypatch, (nx, ny, "full", 3), (9,), SINGLY + ALL_ON)


@pytest.mark.parametrize("seed,holes", [(31, 0.35), (32, 0.7)])
def test_random_independent_masks(seed, holes, monkeypatch):
    """Partial tiles (one to three ice-holding chunks) take the lock while full tiles skip it."""
    _check(monkeypatch, (100, 116, "full", seed, holes), (9,), [(0, 1, 0), (0, 0, 1), (1, 1, 1), (3, 1, 1)])


@pytest.mark.parametrize("prio", [1, 2, 3])
def test_priorities_do_not_starve_lagging_tiles(prio, monkeypatch):
    """Every fourth tile delayed by 10 us per subcycle (CICE_EVP_HIP_RES_DEBUG=8): a raised or a spinning wave must not starve
    a lagging producer on its SIMD.  A starved wait gives up and shows as a fallback, which _run refuses."""
    key = (100, 116, "full", 21)
    assert_bitwise(_run(monkeypatch, (prio, 1, 1), _case(*key), (24,), debug=8), _oracle(key, 24), f"lagging tiles, priorities {prio} vs oracle")


# the split division on the states of tests/test_gpu_resident_range_math.py: b velocities and currents exactly zero on a patch,
# c velocities about 1e-125 there, e2 one cell in 35 with zero velocity, current and strength (nearly every wave mixed)
@pytest.mark.parametrize("which", ["a", "b", "c", "e2"])
@pytest.mark.parametrize("ndte", [2, 7])
def test_split_division_states(which, ndte, monkeypatch):
    dom = "gx3-full"
    want = _state_oracle(dom, which, ndte)
    for sw in ((0, 0, 1), (2, 0, 1)):
        got = _run(monkeypatch, sw, _state(dom, which), (ndte,))
        assert_bitwise(got, want, f"{dom} {which} {ndte}: split division (switches {sw}) vs oracle")
    assert_bitwise(got, _run(monkeypatch, OFF, _state(dom, which), (ndte,)), f"{dom} {which} {ndte}: split division vs all off")


@functools.lru_cache(maxsize=None)
def _still_state(dom):
    """State b (velocities and currents exactly zero on a patch) with nothing left there that could move the ice: forcing and
    stresses zero as well.  Inside the patch both numerators of the momentum step are exactly zero -- outside the window -- until
    the surroundings reach in, one cell per subcycle."""
    dc, geo, fields, tm, um = _state(dom, "b")
    f = {k: np.array(v, copy=True) for k, v in fields.items()}
    still = f["uocnU"] == 0.0
    for k in ("forcexU", "forceyU") + tuple(evp.FIELDS[:12]):
        f[k][still] = 0.0
    return dc, geo, f, tm, um


def test_split_division_takes_both_paths(monkeypatch):
    """The test build counts, per wave, the passes that took the compiler's forms.  With the split off the momentum step's second
    part counts nothing, so the difference between the two runs is the number of second parts that left the cores: none on the
    ordinary state (every second part there ran quot_core); where a patch of ice lies still some waves leave them in every
    subcycle, and the outputs are the oracle's there too."""
    dom, ndte = "gx3-full", 7
    got1, n1 = _run(monkeypatch, (0, 0, 1), _state(dom, "a"), (ndte,), stamps=True)
    got0, n0 = _run(monkeypatch, OFF, _state(dom, "a"), (ndte,), stamps=True)
    assert_bitwise(got1, got0, f"{dom} a: split division vs off, stamps on")
    assert (n1 == n0).all(), "ordinary state: every second part on the cores"
    case = _still_state(dom)
    want = run_oracle(*case, SCAL, ndte)
    got1, n1 = _run(monkeypatch, (0, 0, 1), case, (ndte,), stamps=True)
    got0, n0 = _run(monkeypatch, OFF, case, (ndte,), stamps=True)
    assert_bitwise(got1, want, f"{dom} still patch: split division vs oracle")
    assert_bitwise(got1, got0, f"{dom} still patch: split division vs off")
    left = n1 - n0
    print(f"{dom} still patch: second parts on the compiler's divisions {int(left.sum())} in {int((left > 0).sum())} waves, "
          f"{int((left == ndte).sum())} of them in every subcycle")
    assert (left >= 0).all() and (left <= ndte).all()
    assert (left == ndte).sum() > 0, "no wave took the compiler's divisions under the split: the library path did not run"
