"""CPU: the restatement of the passes after the subcycle loop (tests/tail_ref.py) is pinned where the fixtures can pin it, its
planted errors show, and the library's new entry points fail loudly before anything has been initialised."""
import ctypes as C

import numpy as np
import pytest

import oracle
import tail_ref
from cice_amd import decomp, evp
from common import CGRID_CASES, CGRID_TFOLD_CASES, GoldenCase, bits_equal


@pytest.mark.parametrize("name", CGRID_CASES + CGRID_TFOLD_CASES)
def test_halo_step_reproduces_the_references_strint_arrays(name):
    """The loop's own strintxE / strintyN (oracle.cgrid_subcycle: before evp()'s halo update of them, ice_dyn_evp.F90:1437-1440)
    pushed through tail_ref's halo step equal the arrays the reference's evp() left, bit for bit, ghost cells included -- and
    they do not before it, so the step is what makes them equal."""
    c = GoldenCase(name)
    dom, p, static = c.oracle_domain(), c.oracle_params(), c.cgrid_static()
    moved = False
    for icall in range(1, c.ncalls + 1):
        state, inputs, masks = c.cgrid_inputs(icall)
        for nsub in c.nsub_list:
            out = oracle.cgrid_subcycle(dom, p, nsub, state, inputs, static, masks, visc_method=str(c.d["visc_method"]))
            want = c.cgrid_expected(icall, nsub)
            sx, sy = tail_ref.cgrid_halo(dom, out["strintxE"], out["strintyN"])
            assert bits_equal(sx, want["strintxE"]), f"{name} call {icall} nsub {nsub} strintxE"
            assert bits_equal(sy, want["strintyN"]), f"{name} call {icall} nsub {nsub} strintyN"
            moved = moved or not (bits_equal(out["strintxE"], sx) and bits_equal(out["strintyN"], sy))
    assert moved, f"{name}: the halo update changed nothing"


def tripole_state(seed=5):
    """A 40 x 24 tripole grid cut into 2 x 2 blocks with random fields on every interior cell."""
    rng = np.random.default_rng(seed)
    dc = decomp.Decomp(40, 24, 20, 12, "cyclic", "tripole", 1)
    shape = (len(dc.local_blocks(0)), dc.ny_block, dc.nx_block)
    f = {k: rng.uniform(-1.0, 1.0, shape) for k in ("sx", "sy")}
    f["ai"] = rng.uniform(0.1, 1.0, shape)
    f["ai"][rng.uniform(size=shape) < 0.2] = 0.0
    f["uarea"] = rng.uniform(0.5, 2.0, shape)           # not symmetric in (i, j)
    f["tarea"] = rng.uniform(0.5, 2.0, shape)
    static = dict(earea=rng.uniform(0.5, 2.0, shape), narea=rng.uniform(0.5, 2.0, shape),
                  epm=(rng.uniform(size=shape) < 0.8).astype(np.float64), npm=(rng.uniform(size=shape) < 0.8).astype(np.float64))
    return dc, f, static


def test_planted_errors_show():
    dc, f, static = tripole_state()
    dom, blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
    good = tail_ref.cgrid_tail(dom, blocks, f["sx"], f["sy"], static)
    # the fold sign dropped: the ghost row beyond the fold (and the N faces on it) come out with the other sign
    bad = tail_ref.cgrid_tail(dom, blocks, f["sx"], f["sy"], static, fold_sign=False)
    assert not bits_equal(bad["strintxE"], good["strintxE"]) and not bits_equal(bad["strintyN"], good["strintyN"])
    assert not bits_equal(bad["strintxU"], good["strintxU"])
    # 'N' and 'E' swapped
    bad = tail_ref.cgrid_tail(dom, blocks, f["sx"], f["sy"], static, swap_dirs=True)
    assert not bits_equal(bad["strintxU"], good["strintxU"]) and not bits_equal(bad["strintyU"], good["strintyU"])
    # (i-1, j) and (i, j-1) swapped
    good = tail_ref.strocn_t(dom, blocks, f["sx"], f["sy"], f["ai"], f["uarea"], f["tarea"])
    bad = tail_ref.strocn_t(dom, blocks, f["sx"], f["sy"], f["ai"], f["uarea"], f["tarea"], swap_neighbours=True)
    assert not bits_equal(bad["strocnxT_iavg"], good["strocnxT_iavg"]) and not bits_equal(bad["strocnyT_iavg"], good["strocnyT_iavg"])
    # ... and the halo update matters: without it the cells next to a block edge lose their ghost neighbours
    bad = tail_ref.strocn_t(None, blocks, f["sx"], f["sy"], f["ai"], f["uarea"], f["tarea"])
    assert not bits_equal(bad["strocnxT_iavg"], good["strocnxT_iavg"])


def test_outputs_are_zero_off_the_physical_cells():
    dc, f, static = tripole_state(seed=6)
    dom, blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
    inner = tail_ref._interior(f["sx"].shape, blocks)
    t = tail_ref.cgrid_tail(dom, blocks, f["sx"], f["sy"], static)
    s = tail_ref.strocn_t(dom, blocks, f["sx"], f["sy"], f["ai"], f["uarea"], f["tarea"])
    for a in (t["strintxU"], t["strintyU"], s["strocnxT_iavg"], s["strocnyT_iavg"]):
        assert bits_equal(a[~inner], np.zeros(int((~inner).sum()))) and np.abs(a[inner]).max() > 0


def test_u2t_flux_known_answer():
    """One cell by hand: p25 * (w(i,j) ua(i,j) + w(i-1,j) ua(i-1,j) + w(i,j-1) ua(i,j-1) + w(i-1,j-1) ua(i-1,j-1)) / tarea(i,j)."""
    w = np.arange(1.0, 17.0).reshape(1, 4, 4)
    ua = 1.0 + 0.5 * np.arange(16.0).reshape(1, 4, 4) ** 2
    ta = np.full((1, 4, 4), 3.0)
    out = tail_ref.u2t_flux([(2, 3, 2, 3)], w, ua, ta)
    j, i = 2, 1
    want = 0.25 * (w[0, j, i] * ua[0, j, i] + w[0, j, i - 1] * ua[0, j, i - 1] + w[0, j - 1, i] * ua[0, j - 1, i]
                   + w[0, j - 1, i - 1] * ua[0, j - 1, i - 1]) / 3.0
    assert out[0, j, i] == want and out[0, 0, 0] == 0.0 and out[0, 3, 3] == 0.0


def test_x2ys_known_answer():
    s = np.arange(1.0, 17.0).reshape(1, 4, 4)
    w = 1.0 + np.arange(16.0).reshape(1, 4, 4)
    m = np.ones((1, 4, 4))
    m[0, 2, 1] = 0.0
    j, i = 1, 1
    n = tail_ref.x2ys([(2, 3, 2, 3)], s, w, m, "N")
    assert n[0, j, i] == (s[0, j, i] * w[0, j, i] + 0.0 * s[0, j + 1, i] * w[0, j + 1, i]) / (w[0, j, i] + 0.0 * w[0, j + 1, i])
    e = tail_ref.x2ys([(2, 3, 2, 3)], s, w, m, "E")
    assert e[0, j, i] == (s[0, j, i] * w[0, j, i] + s[0, j, i + 1] * w[0, j, i + 1]) / (w[0, j, i] + w[0, j, i + 1])
    m[:] = 0.0
    assert not tail_ref.x2ys([(2, 3, 2, 3)], s, w, m, "N").any()        # weights sum to 0: the output stays 0


def test_principal_stress_branches():
    puny = 1.0e-11
    st = np.array([puny, np.nextafter(puny, 1.0), 0.0, 2.0])
    out = tail_ref.principal_stress(np.full(4, 3.0), np.full(4, 4.0), np.full(4, 1.5), st, puny)
    for k in ("sig1", "sig2", "sigP"):
        assert out[k][0] == 1.0e30 and out[k][2] == 1.0e30 and out[k][1] != 1.0e30
    assert out["sigP"][3] == -1.5 and out["sig1"][3] == (0.5 * (3.0 + 5.0)) / 2.0 and out["sig2"][3] == (0.5 * (3.0 - 5.0)) / 2.0


@pytest.mark.parametrize("testing", [False, True])
def test_new_entry_points_fail_loudly_before_init(testing):
    lib = evp.load_library(testing=testing)
    a = np.zeros(16)
    p = a.ctypes.data_as(C.POINTER(C.c_double))
    calls = {
        "cice_evp_hip_strocn_t": lambda: lib.cice_evp_hip_strocn_t(p, p, p, p),
        "cice_evp_hip_principal_stress": lambda: lib.cice_evp_hip_principal_stress(C.c_double(1e-11), p, p, p),
        "cice_evp_hip_cgrid_tail": lambda: lib.cice_evp_hip_cgrid_tail(p, p, p, p, C.c_int32(0)),
        "cice_evp_hip_cgrid_dyn_finish_u": lambda: lib.cice_evp_hip_cgrid_dyn_finish_u(p, p, p, p, p, p, p),
        "cice_evp_hip_cgrid_strocn_t": lambda: lib.cice_evp_hip_cgrid_strocn_t(p, p),
    }
    for name, call in calls.items():
        assert call() != 0, f"{name} returned success before cice_evp_hip_init"
        buf = C.create_string_buffer(256)
        lib.cice_evp_hip_last_error(buf, 256)
        assert b"upload" in buf.value or b"initialised" in buf.value, (name, buf.value)
    assert not a.any()
