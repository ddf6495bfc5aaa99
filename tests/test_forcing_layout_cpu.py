"""The numpy restatement of the forcing-layout averages (tests/forcing_layout_ref.py) pinned on hand-worked answers: one
6 x 5 block with the physical cells i = 2..5, j = 2..4 (1-based), distinct areas per location, a(i, j) = 10 i + j."""
from __future__ import annotations

from fractions import Fraction as Fr

import numpy as np
import pytest

from forcing_layout_ref import STENCIL, layout_products, x2y

NX, NY = 6, 5
BLOCKS = [(2, 5, 2, 4)]


def grid():
    ii, jj = np.meshgrid(np.arange(1, NX + 1, dtype=np.float64), np.arange(1, NY + 1, dtype=np.float64))
    area = {"T": (1.0 + 0.0 * ii)[None], "U": (ii + jj)[None], "E": (2 * ii + jj)[None], "N": (ii + 2 * jj)[None]}
    pm = {k: np.ones((1, NY, NX)) for k in "TUEN"}
    a = (10 * ii + jj)[None]
    return a, area, pm


def at(x, i, j):
    return x[0, j - 1, i - 1]


# value at (i, j) = (3, 3) of every new average, worked by hand from area U = i + j, E = 2 i + j, N = i + 2 j, masks 1:
#   'S' = sum(a w) / sum(w), 'F' = p5 (two points) or p25 (four) * sum(a w) / area_target(3, 3)
HAND = {
    ("U", "E"): (Fr(32 * 5 + 33 * 6, 11), Fr(1, 2) * (32 * 5 + 33 * 6) / 9),                                  # S: (3,2) (3,3)
    ("U", "N"): (Fr(23 * 5 + 33 * 6, 11), Fr(1, 2) * (23 * 5 + 33 * 6) / 9),                                  # W: (2,3) (3,3)
    ("E", "U"): (Fr(33 * 9 + 34 * 10, 19), Fr(1, 2) * (33 * 9 + 34 * 10) / 6),                                # N: (3,3) (3,4)
    ("E", "N"): (Fr(23 * 7 + 33 * 9 + 24 * 8 + 34 * 10, 34), Fr(1, 4) * (23 * 7 + 33 * 9 + 24 * 8 + 34 * 10) / 9),   # NW
    ("N", "U"): (Fr(33 * 9 + 43 * 10, 19), Fr(1, 2) * (33 * 9 + 43 * 10) / 6),                                # E: (3,3) (4,3)
    ("N", "E"): (Fr(32 * 7 + 42 * 8 + 33 * 9 + 43 * 10, 34), Fr(1, 4) * (32 * 7 + 42 * 8 + 33 * 9 + 43 * 10) / 9),   # SE
}


@pytest.mark.parametrize("src,dst", sorted(HAND))
@pytest.mark.parametrize("kind", ["S", "F"])
def test_stencil_value_at_a_cell(src, dst, kind):
    a, area, pm = grid()
    got = at(x2y(kind, a, src, dst, area, pm, BLOCKS), 3, 3)
    want = HAND[(src, dst)][0 if kind == "S" else 1]
    assert got == pytest.approx(float(want), rel=1e-15, abs=0.0)


def test_every_new_stencil_is_pinned():
    assert set(HAND) == {k for k in STENCIL if k[0] != "T"}


@pytest.mark.parametrize("src,dst", sorted(STENCIL))
@pytest.mark.parametrize("kind", ["S", "F"])
def test_ghost_cells_are_zero_after_an_average(src, dst, kind):
    a, area, pm = grid()
    out = x2y(kind, a, src, dst, area, pm, BLOCKS)
    ghost = np.ones((1, NY, NX), bool)
    ghost[0, 1:4, 1:5] = False
    assert not out[ghost].any()
    assert (out[~ghost] != 0).all()


@pytest.mark.parametrize("loc", ["T", "U", "E", "N"])
@pytest.mark.parametrize("kind", ["S", "F"])
def test_same_location_copies_the_whole_array(loc, kind):
    a, area, pm = grid()
    a = a + 0.5                                  # ghost cells not 0
    out = x2y(kind, a, loc, loc, area, pm, BLOCKS)
    assert np.array_equal(out.view(np.uint64), a.view(np.uint64))


def test_mask_drops_a_cell_from_the_state_average():
    a, area, pm = grid()
    pm["E"][0, 2, 1] = 0.0                       # epm(2, 3) = 0: E2NS at (3, 3) keeps three cells
    got = at(x2y("S", a, "E", "N", area, pm, BLOCKS), 3, 3)
    assert got == pytest.approx(float(Fr(33 * 9 + 24 * 8 + 34 * 10, 27)), rel=1e-15, abs=0.0)
    # ... and the flux average ignores the mask
    assert at(x2y("F", a, "E", "N", area, pm, BLOCKS), 3, 3) == at(x2y("F", a, "E", "N", area, grid()[2], BLOCKS), 3, 3)


def test_zero_weight_sum_gives_zero_under_S():
    a, area, pm = grid()
    pm["U"][0, 1, 2] = 0.0                       # uvm(3, 2) = uvm(3, 3) = 0: U2ES at (3, 3) has no weight
    pm["U"][0, 2, 2] = 0.0
    out = x2y("S", a, "U", "E", area, pm, BLOCKS)
    assert at(out, 3, 3) == 0.0 and not np.signbit(at(out, 3, 3))
    assert at(out, 4, 3) != 0.0


def test_T_sources_match_the_existing_preparation_formulas():
    """The T sources of the restatement against the formulas the default preparation keeps (evp_prep.hip, evp_cgrid_prep.hip):
    4-point 'S' / 'F' to U, 2-point to E and N."""
    a, area, pm = grid()
    pm["T"][0, 2, 3] = 0.0
    m, w = pm["T"][0], area["T"][0]
    i, j = 3, 2                                  # (0-based column / row of cell (4, 3))
    u = (m[j, i] * a[0, j, i] * w[j, i] + m[j, i + 1] * a[0, j, i + 1] * w[j, i + 1] + m[j + 1, i] * a[0, j + 1, i] * w[j + 1, i]
         + m[j + 1, i + 1] * a[0, j + 1, i + 1] * w[j + 1, i + 1]) / (m[j, i] * w[j, i] + m[j, i + 1] * w[j, i + 1]
                                                                     + m[j + 1, i] * w[j + 1, i] + m[j + 1, i + 1] * w[j + 1, i + 1])
    assert x2y("S", a, "T", "U", area, pm, BLOCKS)[0, j, i] == u
    f = 0.5 * (a[0, j, i] * w[j, i] + a[0, j, i + 1] * w[j, i + 1]) / area["E"][0, j, i]
    assert x2y("F", a, "T", "E", area, pm, BLOCKS)[0, j, i] == f


def test_layout_products_pick_the_grids_of_the_layout():
    a, area, pm = grid()
    t = {"uocn": a, "vocn": a + 1, "strairxT": a + 2, "strairyT": a + 3, "strax": a + 4, "stray": a + 5, "ss_tltx": a + 6,
         "ss_tlty": a + 7}
    b = layout_products("B", False, "B", "C", t, area, pm, BLOCKS)
    assert np.array_equal(b["uocnU"], t["uocn"]) and np.array_equal(b["vocnU"], t["vocn"])        # U -> U: copies
    assert np.array_equal(b["strairxU"], x2y("F", t["strax"], "E", "U", area, pm, BLOCKS))
    assert np.array_equal(b["strairyU"], x2y("F", t["stray"], "N", "U", area, pm, BLOCKS))
    c = layout_products("C", True, "C", "B", t, area, pm, BLOCKS)
    assert np.array_equal(c["uocnE"], t["uocn"]) and np.array_equal(c["vocnN"], t["vocn"] + 0)
    assert np.array_equal(c["vocnE"], x2y("S", t["vocn"], "N", "E", area, pm, BLOCKS))
    assert np.array_equal(c["strairxE"], x2y("F", t["strairxT"], "T", "E", area, pm, BLOCKS))     # calc_strair: atm ignored
    assert np.array_equal(b["ss_tltxU"], t["ss_tltx"]) and np.array_equal(c["ss_tltxE"], t["ss_tltx"])   # at their grid_ocn points
    assert np.array_equal(c["ss_tltyN"], t["ss_tlty"])
    assert np.array_equal(layout_products("C", True, "B", "A", t, area, pm, BLOCKS)["ss_tltyN"],
                          x2y("S", t["ss_tlty"], "U", "N", area, pm, BLOCKS))
