"""GPU (-m gpu): what a launch of the lean on-chip resident B-grid kernel pays beside its subcycles (evp_resident2.hip: the prologue
above the loop and the write-back below it), switch by switch:
  full tiles taking the identity chunk map without the per-CU lock (CICE_EVP_HIP_RES_NOLOCK);
  the final stresses and velocities stored into ONE ping-pong buffer, the one that is current after the call
    (CICE_EVP_HIP_RES_WRITE_ONCE; cur0 ^ (ndte & 1));
  the per-CU record of the partial tiles as one 64-bit word under a compare-and-swap loop instead of the lock
    (CICE_EVP_HIP_RES_LOCK_CAS)
against the oracle and against the kernel with all three off, all 18 outputs -- ghost cells included -- bit for bit (fp64 compared
as uint64 patterns).  None may change a bit: any chunk -> wave map is correct, and the buffer that is not current is written
before it is read by whatever advances the state next -- which the sequences below put to the test: several calls on one state with odd and even counts, a call the streaming kernel runs between resident ones and the
reverse (CICE_EVP_HIP_RES_DECLINE, read at every call), and two calls with the stresses kept on the device under masks that lose
and gain ice in between.  Every call that was meant for the resident kernel asserts tile_variant == 2004 on the rim-wave schedule
and resident_fallbacks == 0; a declined one asserts that another kernel ran."""
import functools

import numpy as np
import pytest

from common import assert_bitwise
from test_gpu_parity import run_oracle
from test_gpu_resident_rim_u import SCAL, _case, _oracle
from cice_amd import evp

pytestmark = pytest.mark.gpu

OFF = (0, 0, 0)                                # (full tiles skip the lock, one write-back, the record under a swap loop): the launch as it was
SINGLY = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
ALL_ON = (1, 1, 1)
SIG = evp.FIELDS[:12]


def _open(monkeypatch, switches, case, debug=None):
    nolock, once, cas = switches
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RES_LOGW", "4")
    monkeypatch.setenv("CICE_EVP_HIP_RES_NOLOCK", str(nolock))
    monkeypatch.setenv("CICE_EVP_HIP_RES_WRITE_ONCE", str(once))
    monkeypatch.setenv("CICE_EVP_HIP_RES_LOCK_CAS", str(cas))
    monkeypatch.setenv("CICE_EVP_HIP_RES_DECLINE", "0")
    if debug is not None:
        monkeypatch.setenv("CICE_EVP_HIP_RES_DEBUG", str(debug))
    dc, geo, fields, tm, um = case
    d, keep = evp.make_dims(dc, 0)
    return evp.EvpHip(d, evp.make_params(SCAL, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"],
                      geo["uarear"], geo["tarea"], keepalive=keep)


def _ran_resident(core, what):
    tmg = core.timings()
    assert tmg["tile_variant"] == 2004, (what, tmg)
    assert tmg["resident_fallbacks"] == 0, (what, tmg)
    assert "edge U-cells in the rim wave" in core.describe_path(), (what, core.describe_path())


def _run(monkeypatch, switches, case, counts, debug=None, decline=None):
    """One EvpHip (test build) on the case (dc, geo, fields, tm, um) with the switches set, subcycle(n) for every n of counts on
    the one state; decline[k]: call k goes through the kernels the resident kernel stands in for."""
    core = _open(monkeypatch, switches, case, debug)
    try:
        core.upload(case[2], case[3], case[4])
        for k, n in enumerate(counts):
            declined = bool(decline and decline[k])
            monkeypatch.setenv("CICE_EVP_HIP_RES_DECLINE", "1" if declined else "0")
            core.subcycle(n)
            core.sync()
            if declined:
                tmg = core.timings()
                assert tmg["tile_variant"] < 2000 or tmg["tile_variant"] >= 3000, (k, tmg)
                assert tmg["resident_fallbacks"] == 0, (k, tmg)
            else:
                _ran_resident(core, f"call {k} of {counts}")
        return core.download()
    finally:
        core.finalize()


def _check(monkeypatch, key, counts, forms, debug=None, decline=None):
    want = _oracle(key, sum(counts))
    assert np.abs(want["uvel"]).max() > 1e-4          # the case moves ice
    off = _run(monkeypatch, OFF, _case(*key), counts, debug, decline)
    assert_bitwise(off, want, f"{key} {counts}: all switches off vs oracle")
    for sw in forms:
        assert_bitwise(_run(monkeypatch, sw, _case(*key), counts, debug, decline), off,
                       f"{key} {counts}: lock skipped {sw[0]}, one write-back {sw[1]}, swap loop {sw[2]} vs all off")


@pytest.mark.parametrize("ndte", [1, 2, 7])
@pytest.mark.parametrize("case", ["full", "caps"])
def test_each_switch_singly_and_all_on(case, ndte, monkeypatch):
    """Odd and even counts: the final state lands in either buffer; ndte = 1 goes from the prologue straight to the write-back."""
    _check(monkeypatch, (100, 116, case, 20261018), (ndte,), SINGLY + [ALL_ON])


@pytest.mark.parametrize("nx,ny", [(15, 15), (31, 16)])
def test_small_cyclic_domains(nx, ny, monkeypatch):
    """One and two tiles whose edge cells have images across the cyclic boundary (corner cells: two), a tile fill that runs
    into the rows and columns outside the arrays, a last tile row with a single U-row."""
    _check(monkeypatch, (nx, ny, "full", 3), (9,), SINGLY + [ALL_ON])
    _check(monkeypatch, (nx, ny, "full", 3), (4,), [ALL_ON])


def test_two_calls_partial_tiles_find_the_previous_launch_in_the_record(monkeypatch):
    """7 then 8 subcycles on partial tiles: the second launch finds the first one's epoch in the per-CU word (and, under the lock,
    its stamp) and starts its counts from zero; switching the form between two cores leaves each its own words."""
    _check(monkeypatch, (100, 116, "full", 32, 0.7), (7, 8), [(0, 0, 1), (1, 0, 1), ALL_ON])


@pytest.mark.parametrize("seed,holes", [(31, 0.35), (32, 0.7)])
def test_random_independent_masks(seed, holes, monkeypatch):
    """Partial tiles (one to three ice-holding chunks) take the lock or the swap loop while full tiles skip it; cells off either
    mask are not written."""
    _check(monkeypatch, (100, 116, "full", seed, holes), (9,), SINGLY + [ALL_ON])
    _check(monkeypatch, (100, 116, "full", seed, holes), (6,), [ALL_ON])


@pytest.mark.parametrize("sw", SINGLY + [ALL_ON])
def test_lagging_tiles(sw, monkeypatch):
    """Every fourth tile delayed by 10 us per subcycle (CICE_EVP_HIP_RES_DEBUG=8): workgroups reach the write-back far apart."""
    key = (100, 116, "full", 21)
    assert_bitwise(_run(monkeypatch, sw, _case(*key), (13,), debug=8), _oracle(key, 13), f"lagging tiles, switches {sw} vs oracle")


@pytest.mark.parametrize("counts", [(7, 8), (8, 7), (7, 8, 5), (1, 1, 2)])
def test_calls_on_one_state(counts, monkeypatch):
    """Two and three calls without an upload in between, odd then even and the reverse: a call reads the buffer the previous one
    left current, whichever it is, and the other one holds older values on the ice."""
    _check(monkeypatch, (100, 116, "caps", 5), counts, SINGLY + [ALL_ON])


@pytest.mark.parametrize("counts,decline", [((7, 8), (0, 1)), ((7, 8), (1, 0)), ((8, 7), (0, 1)), ((7, 4, 5), (0, 1, 0)), ((3, 4, 6), (1, 0, 1))])
def test_resident_and_streaming_calls_on_one_state(counts, decline, monkeypatch):
    """A resident call followed by one the streaming kernel runs on the same device state, and the reverse: the streaming kernel
    reads the current buffer and writes the other one's ice cells before anybody reads them; the resident kernel finds the
    state in whichever buffer the streaming call ended in."""
    _check(monkeypatch, (100, 116, "full", 31, 0.35), counts, [(0, 1, 0), ALL_ON], decline=decline)


# ---- the stresses stay on the device between two calls whose masks differ ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_mask_calls(n1, n2):
    """Call 1 on the holes case; call 2 from its outputs under ANOTHER random pair of masks (cells lose and gain ice), the stresses
    zeroed off the new T-mask and the velocities off the new U-mask as dyn_prep2 leaves them.  Returns the inputs and the oracle's
    outputs of both calls."""
    case1 = _case(100, 116, "full", 31, 0.35)
    dc, geo, fields, tm1, um1 = case1
    tm2, um2 = _case(100, 116, "full", 32, 0.35)[3:5]
    assert ((tm1 != 0) & (tm2 == 0)).any() and ((tm1 == 0) & (tm2 != 0)).any()
    assert ((um1 != 0) & (um2 == 0)).any() and ((um1 == 0) & (um2 != 0)).any()
    out1 = run_oracle(dc, geo, fields, tm1, um1, SCAL, n1)
    fields2 = {k: np.array(v, copy=True) for k, v in fields.items()}
    for k in evp.OUTPUTS:
        fields2[k] = np.array(out1[k], copy=True)
    for k in SIG:                                   # (+0.0 off the mask, as the device zeroes them: x * 0 keeps the sign of x)
        fields2[k] = np.where(tm2 != 0, fields2[k], 0.0)
    for k in ("uvel", "vvel"):
        fields2[k] = np.where(um2 != 0, fields2[k], 0.0)
    out2 = run_oracle(dc, geo, fields2, tm2, um2, SCAL, n2)
    return case1, out1, (dc, geo, fields2, tm2, um2), out2


def _run_two_mask_calls(monkeypatch, sw, n1, n2, decline=(0, 0)):
    case1, out1, case2, out2 = _two_mask_calls(n1, n2)
    core = _open(monkeypatch, sw, case1)
    nonsig = [k for k in evp.OUTPUTS if k not in SIG]
    try:
        core.set_option(evp.OPT_STRESS_RESIDENT, 1)
        got = []
        for k, (case, n, want) in enumerate(((case1, n1, out1), (case2, n2, out2))):
            monkeypatch.setenv("CICE_EVP_HIP_RES_DECLINE", str(decline[k]))
            f = dict(case[2])
            if k == 1:
                f = dict(f, **{s: np.full_like(f[s], np.nan) for s in SIG})      # (kept on the device: the caller's never travel)
            out = core.run(f, case[3], case[4], ndte=n)
            if not decline[k]:
                _ran_resident(core, f"call {k + 1}, switches {sw}")
            assert core.timings()["resident_fallbacks"] == 0
            sig = core.fetch_stresses()
            res = dict({q: out[q] for q in nonsig}, **sig)
            assert_bitwise(res, {q: want[q] for q in res}, f"stresses resident, call {k + 1} ({n} subcycles), switches {sw}, declined {decline}")
            got.append(res)
        assert all(not got[1][s][case2[3] == 0].any() for s in SIG), "stresses survive off the new iceTmask"
        return got
    finally:
        core.finalize()


@pytest.mark.parametrize("n1,n2", [(7, 8), (8, 7), (7, 7)])
def test_stresses_resident_masks_lose_and_gain_ice(n1, n2, monkeypatch):
    """OPT_STRESS_RESIDENT: the second call uploads no stress, zeroes both buffers off its masks and reads the buffer the first
    call left current -- with one write-back the only one that holds the first call's result."""
    off = _run_two_mask_calls(monkeypatch, OFF, n1, n2)
    for sw in ([(0, 1, 0), ALL_ON]):
        got = _run_two_mask_calls(monkeypatch, sw, n1, n2)
        for k in (0, 1):
            assert_bitwise(got[k], off[k], f"stresses resident, call {k + 1}: switches {sw} vs all off")


@pytest.mark.parametrize("decline", [(0, 1), (1, 0)])
def test_stresses_resident_resident_then_streaming(decline, monkeypatch):
    """The same pair of calls with one of them run by the streaming kernel."""
    _run_two_mask_calls(monkeypatch, ALL_ON, 7, 8, decline)
