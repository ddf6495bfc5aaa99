"""C-grid EVP on a tripole / tripoleT grid over several ranks ("marched zone + fold band + frame"): the host plan that shares a rank's
interior cells between the marched kernel (the zone) and the list-driven variants of the five phase kernels (the rest: the band under
the fold, the block edges and the FRAME -- what other ranks receive and what has a ghost image here) -- cice_amd/csrc/cgrid_plan.cpp:
build_cg_march_fold, through the test build's cice_evp_hip_cgrid_march_fold_plan with ranks = 1.  The library asserts its invariants
itself; here they are restated in numpy from the plan's bytes, the marched kernel's items, the rank's fold lists, the halo plan's send
lists and the sent-cell list the planner used.

  1. zone and rest are disjoint and together are the interior cells;
  2. the fold rule: no item FORMS a value at a point on the fold or beyond it, and everything it LOADS lies inside the block's array
     and not above the ghost row beyond the fold;
  3. every interior cell of the rank's fold lists (destination or operand, all four field locations) is a rest cell evaluated at every
     level; an operand >= the rank's cells is a staging slot (< cells + staging slots) and needs no level;
  4. every cell another rank receives in an in-loop exchange (the velocity lists' and the C-grid lists' send sources, the raw fold
     sources for other ranks' staging slots included) and every cell with a ghost image on this rank is a rest cell evaluated at every
     level; the planner's sent-cell list is exactly those send sources;
  5. every value a phase reads at an interior cell is produced by the phase before it; every evaluated cell has its stencil inside
     the array; no phase but stressC_T runs on a ghost cell; the workgroup lists are exactly the workgroups that hold a cell of the phase.
"""
import numpy as np
import pytest

from cice_amd import decomp, evp

REST, S, T, ZONE, U, AVG, FOLDROW = 1, 2, 4, 8, 16, 32, 64
EVERY = REST | S | T | U | AVG
CENTRE, CORNER, EFACE, NFACE = 0, 1, 2, 3
# What cg_strip forms for an item that owns rows ja .. jb, from its loop (evp_cgrid.hip: iterations j = j0 .. jb + 1; levels S and T and the
# two face averages run on row j, levels U and C on row j - 1): (what, field location, first row - ja, last row - jb)
FORMS = [
    ("face -> corner averages of the previous subcycle", CORNER, -2, +1),
    ("E -> N average", NFACE, 0, +1),
    ("N -> E average", EFACE, 0, +1),
    ("shearU", CORNER, -2, +1),
    ("deltaU", CORNER, 0, 0),
    ("stressC_T", CENTRE, -2, +1),
    ("etax2U, stress12U", CORNER, -1, 0),
    ("momentum step, uvelE", EFACE, 0, 0),
    ("momentum step, vvelN", NFACE, 0, 0),
]
# offsets (di, dj) from the evaluating cell, as in evp_cgrid.hip
P3_READS_U = [(0, 0), (0, -1), (-1, 0)]
P3_READS_T = [(0, 0), (1, 0), (0, 1)]
P2_READS_T = [(0, 0), (1, 0), (0, 1), (1, 1)]
P1_READS_S = [(0, 0), (0, -1), (-1, -1), (-1, 0)]
P0_READS_A = [(0, 0), (1, 0), (0, 1)]


def _drop(dc, dropped):
    """dc with the blocks at the (iblock, jblock) positions `dropped` eliminated (land), local indices renumbered"""
    for b in dc.blocks:
        if (b.iblock, b.jblock) in dropped:
            b.owner = -1
    for r in range(dc.nranks):
        for k, b in enumerate(sorted((b for b in dc.blocks if b.owner == r), key=lambda b: b.gid)):
            b.local = k
    return dc


# name -> the decomposition (north boundary filled in by the test)
LAYOUTS = {
    "400x80_cut2x1": lambda ns: decomp.per_rank_blocks(400, 80, 2, "cyclic", ns, proc_shape=(2, 1)),
    "400x160_cut1x2": lambda ns: decomp.per_rank_blocks(400, 160, 2, "cyclic", ns, proc_shape=(1, 2)),
    "400x160_cut2x2": lambda ns: decomp.per_rank_blocks(400, 160, 4, "cyclic", ns, proc_shape=(2, 2)),
    "600x80_cut3x1_blocks2x1": lambda ns: decomp.Decomp(600, 80, 100, 80, "cyclic", ns, 3, (3, 1)),
    # (the block rows go 2 + 1 to the two ranks: the top rank holds the 12 rows at the fold alone.  On a T-fold they leave no zone -- the one
    # window row that fits, rows NY - 6 .. NY - 2, ends on a source row of the fold step -- so that case is 260 x 73, the least that works)
    "260x72_90x30pad_2ranks": lambda ns: decomp.Decomp(260, 73 if ns == "tripoleT" else 72, 90, 30, "cyclic", ns, 2, (1, 2)),
    # an eliminated land block next to the fold: 4 x 2 blocks of 100 x 40 on two ranks, the second block of the top row dropped
    "400x80_land_at_the_fold": lambda ns: _drop(decomp.Decomp(400, 80, 100, 40, "cyclic", ns, 2, (2, 1)), {(2, 2)}),
    "400x320_cut1x4": lambda ns: decomp.per_rank_blocks(400, 320, 4, "cyclic", ns, proc_shape=(1, 4)),
}


def _shift(m, di, dj):
    """cells READ by the cells of m at offset (di, dj) (nothing wraps: the caller has checked the border)"""
    out = np.zeros_like(m)
    ny, nx = m.shape
    src = m[max(0, -dj):ny - max(0, dj), max(0, -di):nx - max(0, di)]
    out[max(0, dj):ny - max(0, -dj), max(0, di):nx - max(0, -di)] = src
    return out


def _at_fold(tfold, loc, jg, NY):
    return jg > NY or (jg == NY and (tfold or loc in (CORNER, NFACE)))


def _check(dc, rank, lengths):
    d, keep = evp.make_dims(dc, rank)
    plan = evp.cgrid_march_fold_plan(d, lengths=lengths, ranks=True)
    if "declined" in plan:
        return plan
    tfold = dc.ns == "tripoleT"
    NY = dc.ny_global
    cells = plan["cells"]
    nb, nyb, nxb = cells.shape
    ncell = cells.size
    blocks = dc.local_blocks(rank)
    interior = np.zeros(cells.shape, dtype=bool)
    for b in blocks:
        interior[b.local, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    # ---- 1. the two sets ----
    zone = np.zeros(cells.shape, dtype=np.int32)
    for blk, c, ja, jb, lo, hi in plan["items"]:
        zone[blk, ja - 1:jb, c - 2 + lo - 1:c - 2 + hi] += 1
    assert zone.max(initial=0) <= 1, "a cell two items own"
    assert np.array_equal(zone == 1, (cells & ZONE) != 0)
    rest = (cells & REST) != 0
    assert not (rest & (zone == 1)).any()
    assert np.array_equal(rest | (zone == 1), interior)
    assert plan["zone_cells"] == int(zone.sum()) and plan["rest_cells"] == int(rest.sum()) > 0
    assert plan["lengths"] == bool(lengths)
    # ---- 2. the fold rule, item by item ----
    by_local = {b.local: b for b in blocks}
    top = {}
    for blk, c, ja, jb, lo, hi in plan["items"]:
        b = by_local[int(blk)]
        grow = lambda j: b.gj0 + (j - b.jlo)
        assert lo >= (3 if lengths else 2) and hi <= 61
        for what, loc, r0, r1 in FORMS:
            for j in (ja + r0, jb + r1):
                assert not _at_fold(tfold, loc, grow(j), NY), (what, "formed on the fold or beyond it", int(blk), j, grow(j))
        i0, i1, j0, j1 = c - 2, c + 61, ja - (6 if lengths else 5), jb + 3
        assert 1 <= i0 and i1 <= nxb and 1 <= j0 and j1 <= nyb, ("a load outside the array", int(blk), i0, i1, j0, j1)
        assert grow(j1) <= NY + 1, ("a load above the ghost row beyond the fold", int(blk), j1)
        top[int(blk)] = max(top.get(int(blk), 0), grow(jb))
    at_fold = [b for b in blocks if b.gj0 + b.gny - 1 == NY]
    assert plan["fold_band_rows"] == max([NY - top.get(b.local, b.gj0 - 1) for b in at_fold], default=0)
    # ---- 3. the fold step's cells: the lists this rank runs ----
    flat, flat_in = cells.reshape(-1), interior.reshape(-1)
    hp = evp.halo_plan(d)
    xp = evp.cgrid_fold_xplan(d)
    assert plan["staging_slots"] == (xp["tail"] if xp["split"] else 0)
    n_fold = 0
    if xp["split"] or hp["fold_rows"] == 1:
        for loc in ("center", "NEcorner", "Eface", "Nface"):
            fl = xp["fold"][loc]
            for k in ("dst", "a", "b"):
                v = fl[k][fl[k] >= 0]
                assert (v < ncell + plan["staging_slots"]).all(), (loc, k, "an operand behind the staging slots")
                if k == "dst":
                    assert (v < ncell).all(), "a fold destination in the staging slots"
                c = v[v < ncell]
                c = c[flat_in[c]]
                n_fold += len(c)
                assert ((flat[c] & EVERY) == EVERY).all(), (loc, k, "a cell of the fold step is not a rest cell at every level")
    assert (n_fold > 0) == bool(at_fold), (n_fold, len(at_fold))
    frow = np.zeros(cells.shape, dtype=bool)
    for b in at_fold:
        frow[b.local, b.jhi - 1, b.ilo - 1:b.ihi] = True
    assert np.array_equal((cells & FOLDROW) != 0, frow)
    assert rest[frow].all()
    # ---- 4. the frame: what leaves the rank, what has a ghost image here ----
    sent = np.unique(np.concatenate([hp["send_src"], xp["send_src"]]).astype(np.int64))
    sent = sent[(sent >= 0) & (sent < ncell)]
    assert np.array_equal(np.asarray(plan["sent"], dtype=np.int64), sent), "the planner's sent-cell list is not the plans' send sources"
    assert len(sent) > 0
    assert flat_in[sent].all(), "a sent cell that is no interior cell"
    assert ((flat[sent] & EVERY) == EVERY).all(), "a sent cell is not a rest cell at the level that produces its field"
    imaged = np.unique(hp["local_src"][hp["local_src"] >= 0].astype(np.int64))
    assert flat_in[imaged].all() and ((flat[imaged] & EVERY) == EVERY).all(), "a cell with a ghost image is not a rest cell at every level"
    assert plan["frame_cells"] == len(np.union1d(sent, imaged))
    # ---- 5a. stencils inside the array (checked first: the shifts below must not wrap) ----
    sc = (cells & (S | U | AVG | REST)) != 0
    assert not (sc[:, 0, :].any() or sc[:, -1, :].any() or sc[:, :, 0].any() or sc[:, :, -1].any()), "a stencil outside the array"
    tc = (cells & T) != 0
    assert not (tc[:, 0, :].any() or tc[:, :, 0].any()), "phase 1 loads outside the array"
    assert not (sc & ~interior).any(), "a phase other than stressC_T on a ghost cell"
    # ---- 5b. every level's reads are covered ----
    for b in range(nb):
        for reads, readers, need, what in ((P3_READS_U, rest[b], U, "stress12U of phase 3"), (P3_READS_T, rest[b], T, "stresspT of phase 3"),
                                           (P2_READS_T, (cells[b] & U) != 0, T, "etax2T of phase 2"), ([(0, 0)], (cells[b] & U) != 0, S, "shearU of phase 2"),
                                           (P1_READS_S, tc[b], S, "shearU of phase 1"), (P0_READS_A, (cells[b] & S) != 0, AVG, "the averages of phase 0"),
                                           ([(0, 0)], rest[b], AVG, "the averages of phase 3")):
            for di, dj in reads:
                r = _shift(readers, di, dj) & interior[b]
                assert not (r & ((cells[b] & need) == 0)).any(), (what, di, dj)
    for b in blocks:       # the reference's extra T row and column (stress12T of the ghost cells i = ihi + 1, j = jhi + 1)
        assert tc[b.local, b.jlo - 1:b.jhi + 1, b.ihi].all() and tc[b.local, b.jhi, b.ilo - 1:b.ihi + 1].all()
    assert int((tc & ~interior).sum()) == sum((b.ihi - b.ilo + 2) + (b.jhi - b.jlo + 2) - 1 for b in blocks), "phase 1 on other ghost cells"
    # ---- 5c. the workgroup lists ----
    gx, gy = -(-nxb // 64), -(-nyb // 4)
    for k, bit in enumerate((S, T, U, REST, AVG)):
        bb, jj, ii = np.nonzero(cells & bit)
        want = np.unique((bb * gy + jj // 4) * gx + ii // 64)
        assert np.array_equal(np.asarray(plan["wg"][k]), want), k
    return plan


@pytest.mark.parametrize("lengths", [1, 0])
@pytest.mark.parametrize("ns", ["tripole", "tripoleT"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_march_fold_ranks_plan_invariants(layout, ns, lengths):
    dc = LAYOUTS[layout](ns)
    for rank in range(dc.nranks):
        plan = _check(dc, rank, lengths)
        assert "declined" not in plan, (rank, plan)
        assert plan["zone_cells"] > 0 and len(plan["items"]) > 0, rank
        has_fold = any(b.gj0 + b.gny - 1 == dc.ny_global for b in dc.local_blocks(rank))
        assert (plan["fold_band_rows"] > 0) == has_fold, (rank, plan["fold_band_rows"])


@pytest.mark.parametrize("ns", ["tripole", "tripoleT"])
def test_march_fold_ranks_plan_y_cut_lower_ranks_are_zone_and_frame(ns):
    """400 x 320 cut in y over four ranks: the three lower ranks hold no fold rows -- zone + frame, every fold list empty, no band; the
    top rank runs the whole fold step and has a band"""
    dc = LAYOUTS["400x320_cut1x4"](ns)
    for rank in range(4):
        d, keep = evp.make_dims(dc, rank)
        plan = _check(dc, rank, 1)
        assert "declined" not in plan, (rank, plan)
        n_fold = sum(len(evp.cgrid_fold_xplan(d)["fold"][loc]["dst"]) for loc in ("center", "NEcorner", "Eface", "Nface"))
        if rank < 3:
            assert n_fold == 0 and plan["fold_band_rows"] == 0 and not (plan["cells"] & FOLDROW).any(), rank
            assert plan["staging_slots"] == 0
        else:
            assert n_fold > 0 and plan["fold_band_rows"] >= (3 if ns == "tripoleT" else 2), rank


def test_march_fold_ranks_plan_x_cut_uses_the_fold_exchange():
    """400 x 80 cut 2 x 1: the fold rows have two owners -- operands in the staging slots, raw fold sources among the sent cells"""
    dc = LAYOUTS["400x80_cut2x1"]("tripole")
    for rank in range(2):
        d, keep = evp.make_dims(dc, rank)
        plan = _check(dc, rank, 1)
        xp = evp.cgrid_fold_xplan(d)
        assert xp["split"] and plan["staging_slots"] == xp["tail"] > 0
        ncell = plan["cells"].size
        assert any((xp["fold"][loc][k] >= ncell).any() for loc in xp["fold"] for k in ("a", "b")), "no operand in the staging slots"
        nghost = int(xp["peer_nghost_send"].sum())
        assert len(xp["send_src"]) > nghost, "no raw fold source is sent"


def test_march_fold_ranks_plan_a_piece_too_thin_declines_beside_a_rank_that_plans():
    """A cut in x cannot mix ranks with and without a zone: every rank's arrays are as wide as the widest piece (a narrower last piece is
    padded), and a rectangle needs the array width, not the piece's -- 3 x 1 cuts of 80 rows: no rank has a zone up to 266 columns
    (pieces of 89, 89, 88), every rank has one from 268 (90, 90, 88).  A cut in y can: 400 x 24 tripoleT cut 1 x 2 leaves each rank 12
    rows, one window row of 5 -- a zone on the lower rank; on the upper one its top row NY - 2 is a source of the T-fold's fold step,
    and nothing is left.  The GPU test runs this cut with the marching and the non-marching rank side by side."""
    for nx, want in ((266, False), (268, True)):
        dc = decomp.per_rank_blocks(nx, 80, 3, "cyclic", "tripole", proc_shape=(3, 1))
        for rank in range(3):
            assert ("declined" not in _check(dc, rank, 1)) == want, (nx, rank)
    dc = decomp.per_rank_blocks(400, 24, 2, "cyclic", "tripoleT", proc_shape=(1, 2))
    low, high = _check(dc, 0, 1), _check(dc, 1, 1)
    assert "declined" not in low and low["zone_cells"] > 0 and low["fold_band_rows"] == 0
    assert "no rectangle" in high["declined"], high


def test_march_fold_plan_one_rank_question_still_declines_several_ranks():
    dc = LAYOUTS["400x160_cut1x2"]("tripole")
    for rank in range(2):
        d, keep = evp.make_dims(dc, rank)
        assert "several ranks" in evp.cgrid_march_fold_plan(d)["declined"]
        assert "declined" not in evp.cgrid_march_fold_plan(d, ranks=True)
