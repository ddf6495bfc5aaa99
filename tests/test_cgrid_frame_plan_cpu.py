"""C-grid EVP on several ranks: the host plan that shares a rank's interior cells between the marched kernel (the zone) and the
frame variants of the three fused kernels (cice_amd/csrc/halo_plan.cpp: build_cg_frame), checked on the CPU through the test
build's cice_evp_hip_cgrid_frame_plan.  The library asserts the same invariants itself; here they are restated in numpy from the
plan's bytes, the marched kernel's items and the halo plan's lists.

  1. zone and frame are disjoint and together are the interior cells;
  2. every cell a peer receives, and every cell with a ghost image on this rank, is a frame cell;
  3. every shearU / etax2T (and new stresspT / stressmT) a frame cell reads at an interior cell is produced by the level that
     runs before -- level T on the T cells around the cell's three corners, level S at the corners levels T and C read;
  4. every cell a workgroup evaluates has its stencil inside the block's array, and the workgroup lists are exactly the
     workgroups that hold such a cell.
"""
import numpy as np
import pytest

from cice_amd import decomp, evp

FRAME, S, T, ZONE = 1, 2, 4, 8
# offsets (di, dj) from the evaluating cell, as in evp_cgrid.hip: level C reads etax2T at the four T cells around its own, south and
# west corner (the east and north neighbour, whose new stresses it reads too, are among them) and shearU at those three corners;
# level T reads shearU at its own, south, south-west and west corner
C_READS_T = [(0, 0), (1, 0), (0, 1), (1, 1), (0, -1), (1, -1), (-1, 0), (-1, 1)]
C_READS_S = [(0, 0), (0, -1), (-1, 0)]
T_READS_S = [(0, 0), (0, -1), (-1, -1), (-1, 0)]

# (nx, ny, ranks in x and y, blocks per rank in x and y or None); interior rows per block 216 = 5 * 42 + 6 where a zone forms
CASES = {
    "cut2x1": (400, 216, (2, 1), None),
    "cut1x2": (400, 432, (1, 2), None),
    "cut2x2": (400, 432, (2, 2), None),
    "cut3x1": (600, 216, (3, 1), None),
    "cut2x2_blocks2x2": (800, 864, (2, 2), (2, 2)),
    "cut2x1_blocks2x2": (800, 432, (2, 1), (2, 2)),
    "no_zone": (100, 60, (2, 1), None),                 # blocks 50 wide: narrower than a strip, everything is frame
}


def _decomp(nx, ny, shape, bpr):
    world = shape[0] * shape[1]
    dc = decomp.per_rank_blocks(nx, ny, world, "cyclic", "closed", proc_shape=shape)
    if bpr:
        dc = decomp.Decomp(nx, ny, -(-dc.block_size_x // bpr[0]), -(-dc.block_size_y // bpr[1]), "cyclic", "closed", world, dc.proc_shape)
    return dc, world


def _shift(m, di, dj):
    """cells READ by the cells of m at offset (di, dj): out[j + dj, i + di] = m[j, i] (nothing wraps: the caller has checked the
    border)."""
    out = np.zeros_like(m)
    ny, nx = m.shape
    src = m[max(0, -dj):ny - max(0, dj), max(0, -di):nx - max(0, di)]
    out[max(0, dj):ny - max(0, -dj), max(0, di):nx - max(0, -di)] = src
    return out


def _check_rank(dc, rank, expect_zone):
    d, keep = evp.make_dims(dc, rank)
    plan = evp.cgrid_frame_plan(d)
    assert plan is not None
    halo = evp.halo_plan(d)
    cells = plan["cells"]
    nb, nyb, nxb = cells.shape
    blocks = dc.local_blocks(rank)
    assert nb == len(blocks)
    interior = np.zeros(cells.shape, dtype=bool)
    for b in blocks:
        interior[b.local, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    # ---- 1. the two sets ----
    zone = np.zeros(cells.shape, dtype=np.int32)
    for blk, c, ja, jb, lo, hi in plan["items"]:
        zone[blk, ja - 1:jb, c - 2 + lo - 1:c - 2 + hi] += 1
    assert zone.max(initial=0) <= 1, "a cell two items own"
    assert np.array_equal(zone == 1, (cells & ZONE) != 0)
    frame = (cells & FRAME) != 0
    assert not (frame & (zone == 1)).any()
    assert np.array_equal(frame | (zone == 1), interior)
    assert plan["zone_cells"] == int(zone.sum()) and plan["frame_cells"] == int(frame.sum())
    assert (plan["zone_cells"] > 0) == expect_zone, (plan["zone_cells"], expect_zone)
    if expect_zone:
        assert plan["zone_cells"] > plan["frame_cells"], "the marched kernel should own most of such a rank"
    # ---- 2. what leaves the rank or has an image on it belongs to the frame ----
    flat = frame.reshape(-1)
    assert len(halo["send_src"]) > 0
    assert flat[halo["send_src"]].all(), "a cell another rank receives is a zone cell"
    src = halo["local_src"][halo["local_src"] >= 0]
    assert flat[src].all(), "a cell with a ghost image is a zone cell"
    # ---- 4a. stencils inside the array (checked first: the shifts below must not wrap) ----
    sc = (cells & (S | FRAME)) != 0
    assert not (sc[:, 0, :].any() or sc[:, -1, :].any() or sc[:, :, 0].any() or sc[:, :, -1].any()), "a stencil outside the array"
    tc = (cells & T) != 0
    assert not (tc[:, 0, :].any() or tc[:, :, 0].any()), "level T loads outside the array"
    assert not (sc & ~interior).any(), "level S or C on a ghost cell"
    # ---- 3. every intermediate a level reads at an interior cell comes from the level before ----
    for b in range(nb):
        for reads, readers, need, what in ((C_READS_T, frame[b], T, "etax2T"), (C_READS_S, frame[b], S, "shearU of level C"),
                                           (T_READS_S, tc[b], S, "shearU of level T")):
            for di, dj in reads:
                r = _shift(readers, di, dj) & interior[b]
                assert not (r & ((cells[b] & need) == 0)).any(), (what, di, dj)
    # the reference's extra T row and column (stress12T of the ghost cells i = ihi + 1, j = jhi + 1)
    for b in blocks:
        assert tc[b.local, b.jlo - 1:b.jhi + 1, b.ihi].all() and tc[b.local, b.jhi, b.ilo - 1:b.ihi + 1].all()
    assert int((tc & ~interior).sum()) == sum((b.ihi - b.ilo + 2) + (b.jhi - b.jlo + 2) - 1 for b in blocks), "level T on other ghost cells"
    # ---- 4b. the workgroup lists: exactly the 64 x 4 workgroups that hold a cell of the level ----
    gx, gy = -(-nxb // 64), -(-nyb // 4)
    for k, bit in enumerate((S, T, FRAME)):
        bb, jj, ii = np.nonzero(cells & bit)
        want = np.unique((bb * gy + jj // 4) * gx + ii // 64)
        assert np.array_equal(np.asarray(plan["wg"][k]), want), k
    return plan


@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_plan_invariants(case):
    nx, ny, shape, bpr = CASES[case]
    dc, world = _decomp(nx, ny, shape, bpr)
    for rank in range(world):
        plan = _check_rank(dc, rank, expect_zone=(case != "no_zone"))
        if case == "no_zone":
            assert len(plan["items"]) == 0 and plan["zone_cells"] == 0


@pytest.mark.parametrize("rows", [5 * k + 6 for k in (10, 11, 23, 42)])
def test_frame_plan_rows_5k_plus_6(rows):
    """interior row counts 5 k + 6: the last window row of the marched kernel's rectangle ends one row short of the block's top"""
    dc, world = _decomp(300, rows, (2, 1), None)
    for rank in range(world):
        b = dc.local_blocks(rank)[0]
        assert b.jhi - b.jlo + 1 == rows
        _check_rank(dc, rank, expect_zone=True)


def test_frame_plan_declines_on_one_rank():
    """no peers: nothing to plan -- the one-launch schedule serves such a rank, and its plan is what it was"""
    dc = decomp.single_block(400, 216, "cyclic", "closed")
    d, keep = evp.make_dims(dc, 0)
    assert evp.cgrid_frame_plan(d) is None
    sp = evp.cgrid_strip_plan(d)
    assert len(sp["items"]) > 0 and sp["in_zone"].any()
