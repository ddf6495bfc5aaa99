"""C-grid EVP on a grid WITHOUT a fold over several ranks, visc_method = avg_strength ("zone marched + frame" with the five list-driven
phase kernels on the frame): the plan build_cg_march_fold (cice_amd/csrc/cgrid_plan.cpp) makes for such a rank when it is asked the
several-ranks question -- through the test build's cice_evp_hip_cgrid_march_fold_plan with ranks = 1.  The layouts are those of
tests/test_gpu_zz_cgrid_march_ranks.py.  The library asserts its invariants itself; here they are restated in numpy from the plan's
bytes, the marched kernel's items and the halo plan's lists, the read table walked as tests/test_cgrid_march_fold_ranks_plan_cpu.py
walks it:

  1. zone and rest are disjoint and together are the interior cells;
  2. every cell another rank receives and every cell with a ghost image on this rank is a rest cell, evaluated at every level -- the
     frame as build_cg_frame defines it;
  3. every value a phase reads at an interior cell is produced where the read table says; no phase but stressC_T runs on a ghost
     cell; everything the marched kernel loads lies inside the block's array;
  4. no fold: no band rows, no fold-row cells, no staging slots.

On one rank, or asked the one-rank question, a grid without a fold declines with the text it always had."""
import numpy as np
import pytest

from cice_amd import decomp, evp
from test_cgrid_march_fold_ranks_plan_cpu import (AVG, EVERY, FOLDROW, P0_READS_A, P1_READS_S, P2_READS_T, P3_READS_T, P3_READS_U, REST, S, T, U,
                                                  ZONE, _shift)

LAYOUTS = {
    "400x216_cut2x1": lambda: decomp.per_rank_blocks(400, 216, 2, "cyclic", "closed", proc_shape=(2, 1)),
    "400x432_cut1x2": lambda: decomp.per_rank_blocks(400, 432, 2, "cyclic", "closed", proc_shape=(1, 2)),
    "400x432_cut2x2": lambda: decomp.per_rank_blocks(400, 432, 4, "cyclic", "closed", proc_shape=(2, 2)),
    "600x216_cut3x1": lambda: decomp.per_rank_blocks(600, 216, 3, "cyclic", "closed", proc_shape=(3, 1)),
}
DECLINE = "no tripole fold (the one-launch schedule marches such a grid)"


def _check(dc, rank, lengths):
    d, keep = evp.make_dims(dc, rank)
    plan = evp.cgrid_march_fold_plan(d, lengths=lengths, ranks=True)
    assert "declined" not in plan, (rank, plan)
    cells = plan["cells"]
    nb, nyb, nxb = cells.shape
    blocks = dc.local_blocks(rank)
    interior = np.zeros(cells.shape, dtype=bool)
    for b in blocks:
        interior[b.local, b.jlo - 1:b.jhi, b.ilo - 1:b.ihi] = True
    # ---- 1. the two sets ----
    zone = np.zeros(cells.shape, dtype=np.int32)
    for blk, c, ja, jb, lo, hi in plan["items"]:
        zone[blk, ja - 1:jb, c - 2 + lo - 1:c - 2 + hi] += 1
        assert lo >= (3 if lengths else 2) and hi <= 61
        # (what cg_strip loads for the item: cgrid_plan.h, strip_footprint)
        i0, i1, j0, j1 = c - 2, c + 61, ja - (6 if lengths else 5), jb + 3
        assert 1 <= i0 and i1 <= nxb and 1 <= j0 and j1 <= nyb, ("a load outside the array", int(blk), i0, i1, j0, j1)
    assert zone.max(initial=0) == 1, "no zone, or a cell two items own"
    assert np.array_equal(zone == 1, (cells & ZONE) != 0)
    rest = (cells & REST) != 0
    assert not (rest & (zone == 1)).any()
    assert np.array_equal(rest | (zone == 1), interior)
    assert plan["zone_cells"] == int(zone.sum()) > 0 and plan["rest_cells"] == int(rest.sum()) > 0
    assert plan["lengths"] == bool(lengths)
    # ---- 2. the frame ----
    flat, flat_in = cells.reshape(-1), interior.reshape(-1)
    hp = evp.halo_plan(d)
    sent = np.unique(hp["send_src"].astype(np.int64))
    sent = sent[(sent >= 0) & (sent < cells.size)]
    assert len(sent) > 0 and np.array_equal(np.asarray(plan["sent"], dtype=np.int64), sent)
    imaged = np.unique(hp["local_src"][hp["local_src"] >= 0].astype(np.int64))
    for what, c in (("a cell another rank receives", sent), ("a cell with a ghost image here", imaged)):
        assert flat_in[c].all() and ((flat[c] & EVERY) == EVERY).all(), what + " is not a rest cell evaluated at every level"
    assert plan["frame_cells"] == len(np.union1d(sent, imaged)) > 0
    # ---- 3. the read table ----
    sc = (cells & (S | U | AVG | REST)) != 0
    assert not (sc[:, 0, :].any() or sc[:, -1, :].any() or sc[:, :, 0].any() or sc[:, :, -1].any()), "a stencil outside the array"
    tc = (cells & T) != 0
    assert not (tc[:, 0, :].any() or tc[:, :, 0].any()), "phase 1 loads outside the array"
    assert not (sc & ~interior).any(), "a phase other than stressC_T on a ghost cell"
    assert ((cells[rest] & EVERY) == EVERY).all(), "a rest cell without its own levels"
    for b in range(nb):
        for reads, readers, need, what in ((P3_READS_U, rest[b], U, "stress12U of phase 3"), (P3_READS_T, rest[b], T, "stresspT of phase 3"),
                                           (P2_READS_T, (cells[b] & U) != 0, T, "etax2T of phase 2"),
                                           # (visc_method = avg_strength: phase 2 reads deltaU of its own corner, which phase 0 makes)
                                           ([(0, 0)], (cells[b] & U) != 0, S, "shearU / deltaU of phase 2"),
                                           (P1_READS_S, tc[b], S, "shearU of phase 1"), (P0_READS_A, (cells[b] & S) != 0, AVG, "the averages of phase 0"),
                                           ([(0, 0)], rest[b], AVG, "the averages of phase 3")):
            for di, dj in reads:
                r = _shift(readers, di, dj) & interior[b]
                assert not (r & ((cells[b] & need) == 0)).any(), (what, di, dj)
    for b in blocks:       # the reference's extra T row and column (stress12T of the ghost cells i = ihi + 1, j = jhi + 1)
        assert tc[b.local, b.jlo - 1:b.jhi + 1, b.ihi].all() and tc[b.local, b.jhi, b.ilo - 1:b.ihi + 1].all()
    assert int((tc & ~interior).sum()) == sum((b.ihi - b.ilo + 2) + (b.jhi - b.jlo + 2) - 1 for b in blocks), "phase 1 on other ghost cells"
    gx, gy = -(-nxb // 64), -(-nyb // 4)
    for k, bit in enumerate((S, T, U, REST, AVG)):
        bb, jj, ii = np.nonzero(cells & bit)
        assert np.array_equal(np.asarray(plan["wg"][k]), np.unique((bb * gy + jj // 4) * gx + ii // 64)), k
    # ---- 4. no fold ----
    assert plan["fold_band_rows"] == 0 and plan["staging_slots"] == 0 and not (cells & FOLDROW).any()
    return plan


@pytest.mark.parametrize("lengths", [1, 0])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_frame_phases_plan_invariants(layout, lengths):
    dc = LAYOUTS[layout]()
    for rank in range(dc.nranks):
        plan = _check(dc, rank, lengths)
        # the frame is a ring: a block loses at most one column and one row of windows (29 x 5 owned cells each) on every side
        (b,) = dc.local_blocks(rank)
        assert plan["zone_cells"] >= (b.ihi - b.ilo + 1 - 2 * 29) * (b.jhi - b.jlo + 1 - 2 * 5), (rank, plan["zone_cells"], plan["rest_cells"])


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_one_rank_question_still_declines_a_grid_without_a_fold(layout):
    dc = LAYOUTS[layout]()
    for rank in range(dc.nranks):
        d, keep = evp.make_dims(dc, rank)
        assert evp.cgrid_march_fold_plan(d)["declined"] == DECLINE


@pytest.mark.parametrize("ns", ["closed", "cyclic"])
def test_one_rank_without_a_fold_still_declines_either_way(ns):
    d, keep = evp.make_dims(decomp.single_block(400, 216, "cyclic", ns), 0)
    for ranks in (False, True):
        assert evp.cgrid_march_fold_plan(d, ranks=ranks)["declined"] == DECLINE
