"""CPU: what keeps tests/test_gpu_call_chain.py honest.  The oracle's chain (tests/evp_call_chain.py), every stage fed by the one
before, reproduces the post-loop arrays of every fixture -- so the GPU chain is compared with a chain, not with stages that were
each handed the reference's inputs.  And the synthetic cases can see what they are there to see: a stale ghost velocity changes
divu in every block that reads one, dyn_finish keeps its sentinel on some U-cells and overwrites it on others, ice moves on the
fold rows."""
import numpy as np
import pytest

import evp_call_chain as cc
import oracle
from common import GoldenCase, assert_bitwise, bits_equal, tfold_untouched
from test_oracle_golden import check_prep_products

FIXTURES = cc.chain_fixtures()


def test_every_bgrid_fixture_runs_the_chain():
    from common import GOLDEN_CASES, TFOLD_CASES
    assert FIXTURES == GOLDEN_CASES + TFOLD_CASES and len(FIXTURES) >= 15
    for n in FIXTURES:
        c = GoldenCase(n)
        assert cc.post_counts(c) == c.nsub_list, n          # every subcycle count of a fixture has post-loop outputs
        assert all(f"pr{k:02d}_aice" in c.d for k in range(1, c.ncalls + 1)), n


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_chain_reproduces_the_fixture(name):
    c = GoldenCase(name)
    keep = tfold_untouched(c) if c.ns == "tripoleT" else None
    moved = 0.0
    for icall in range(1, c.ncalls + 1):
        for nsub in cc.post_counts(c):
            what = f"{name} call {icall} nsub {nsub}"
            prep, got = cc.oracle_fixture_chain(c, icall, nsub)
            check_prep_products(c, icall, prep, f"prep: {what}")
            cc.assert_stage(got["loop"], c.expected(icall, nsub), f"loop: {what}", keep)
            tag = f"o{icall:02d}n{nsub:04d}_"
            assert_bitwise(got["deformations"], {k: c.d[tag + k] for k in cc.POST}, f"deformations: {what}")
            assert_bitwise(got["dyn_finish"], {k: c.d[tag + k] for k in ("strocnxU", "strocnyU")}, f"dyn_finish: {what}")
            moved = max(moved, float(np.abs(got["deformations"]["divu"]).max()))
            # the east and north fringe T-cells are part of the comparison and not empty
            fringe = np.zeros(c.d["tarea"].shape, bool)
            for b in range(c.nblocks):
                ilo, ihi, jlo, jhi = [int(v) for v in c.blk[b, :4]]
                fringe[b, jlo - 1:jhi + 1, ihi] = True
                fringe[b, jhi, ilo - 1:ihi + 1] = True
            if nsub == c.ndte:
                assert np.abs(c.d[tag + "divu"][fringe]).max() > 0, f"{what}: no divu on the fringe cells"
    assert moved > 0


@pytest.mark.parametrize("name", list(cc.SYNTH_CASES))
def test_synthetic_cases_can_see_what_they_are_for(name):
    case = cc.synth_case(name)
    edge = cc.edge_blocks_with_ice(case)
    assert edge, "no block with ice on its west or south edge"
    for ndte in cc.SYNTH_NDTE:
        want = case.oracle(ndte)
        u, v = want["loop"]["uvel"], want["loop"]["vvel"]
        assert np.abs(u).max() > 1e-4
        # a stale ghost cell: divu changes in every block that has ice on its west or south edge
        stale = oracle.deformations(case.dom, case.prm, cc.zero_ghosts(case, u), cc.zero_ghosts(case, v), case.static, case.post_geo, case.tm)
        diff = stale["divu"].view(np.uint64) != want["deformations"]["divu"].view(np.uint64)
        for b in edge:
            assert diff[b].any(), f"{case.name} ndte {ndte}: block {b} would not notice a stale ghost velocity"
        # dyn_finish: the sentinel survives on some U-cells and not on others
        for k, s in zip(("strocnxU", "strocnyU"), cc.SENTINEL):
            kept = want["dyn_finish"][k] == s
            assert kept.any() and (~kept).any(), (case.name, k)
            # ... it survives exactly off the interior ice U-cells
            inter = np.zeros(kept.shape, bool)
            for b, (ilo, ihi, jlo, jhi) in enumerate(case.blocks):
                inter[b, jlo - 1:jhi, ilo - 1:ihi] = True
            assert bits_equal(~kept, inter & (case.um != 0)), (case.name, k)
        if cc.is_fold(case.ns):
            assert cc.top_rows_move(case, ndte) > 0, "no ice moves on the fold rows"
    # the two counts end on different states: neither is a repeat of the other
    assert not bits_equal(case.oracle(9)["loop"]["uvel"], case.oracle(7)["loop"]["uvel"])


def test_synthetic_cases_cover_what_the_table_says():
    full, caps, holes = (cc.synth_case(n) for n in ("closed full 1blk", "closed caps 25x29", "closed holes 30x40"))
    assert len(full.blocks) == 1 and full.prep_in and caps.prep_in and not holes.prep_in
    assert len(caps.blocks) == 16 and len(holes.blocks) == 12
    # 30 x 40 blocks on 100 x 116: the last block of a row and of a column is padded
    assert {b[1] - b[0] + 1 for b in holes.blocks} == {30, 10} and {b[3] - b[2] + 1 for b in holes.blocks} == {40, 36}
    # independent holes: ice T-cells without an ice U-cell and the other way round
    assert ((holes.tm != 0) & (holes.um == 0)).any() and ((holes.tm == 0) & (holes.um != 0)).any()
    # the preparation of the closed cases gains and loses ice against the previous mask
    prev = full.prep_in[2]["iceUmask"]
    assert ((prev != 0) & (full.um == 0)).any() and ((prev == 0) & (full.um != 0)).any()
    assert 0.2 < (caps.tm != 0).mean() < 0.6


def test_two_call_case_loses_ice():
    """The pair of calls of test_gpu_call_chain.py::test_two_calls_where_cells_lose_their_ice."""
    t = cc.two_calls()
    b = t.base
    lost_t, lost_u = (b.tm != 0) & (t.tm2 == 0), (b.um != 0) & (t.um2 == 0)
    assert lost_t.sum() >= 10 and lost_u.sum() >= 10
    # the cells that lose their ice held something after call 1: stresses, velocities and diagnostics that call 2 must not keep
    assert np.abs(t.out1["stressp_1"][lost_t]).max() > 0 and np.abs(t.out1["uvel"][lost_u]).max() > 0
    assert np.abs(t.out1["strintxU"][lost_u]).max() > 0
    loop = t.want2["loop"]
    for k in cc.SIG:
        assert not loop[k][t.tm2 == 0].any(), k
    for k in ("strintxU", "strintyU", "taubxU", "taubyU"):
        assert (loop[k][t.um2 == 0] == t.off).all(), k                  # the reference leaves the caller's values off the ice
    assert np.abs(loop["strintxU"][t.um2 != 0]).max() > 0 and not bits_equal(loop["uvel"], t.out1["uvel"])
    for k, s in zip(("strocnxU", "strocnyU"), cc.SENTINEL):
        kept = t.want2["dyn_finish"][k] == s
        assert kept.any() and (~kept).any() and kept[lost_u].all(), k


# ---- the extended restatement of the post-loop kernels (tests/post_loop_ref.py) ------------------------------------------------
def _fused_inputs():
    """What the fused-mode GPU test feeds the restatement, with the oracle's velocities in the device's place."""
    case = cc.synth_case(cc.FUSED_CASE)
    want = case.oracle(cc.FUSED_NDTE)
    return case, want, want["loop"]["uvel"], want["loop"]["vvel"]


def test_fp64_oracle_lies_within_the_bound_of_the_extended_restatement():
    import post_loop_ref as R
    case, want, u, v = _fused_inputs()
    got = dict(want["deformations"], **want["dyn_finish"])
    worst = R.check(got, u, v, case.static, case.post_geo, case.dyn, case.scal, case.blocks, case.tm, case.um, cc.SENTINEL, "fp64 oracle")
    print("\nfp64 oracle, worst |error| / bound:", {k: round(x, 3) for k, x in worst.items()})
    assert all(0 < x <= 1 for x in worst.values()), worst          # inside, and not by being compared with itself
    assert set(worst) == set(R.ROUNDINGS)


def test_the_bound_is_not_vacuous():
    """u at (i-1, j) and (i, j-1) swapped in the restatement: the fp64 oracle leaves the bound on more than half of the ice T-cells."""
    import post_loop_ref as R
    case, want, u, v = _fused_inputs()
    on = R.t_list(case.blocks, case.tm)
    wrong = R.deform(u, v, case.static, case.post_geo["dxU"], case.post_geo["dyU"], case.post_geo["tarear"], case.scal["e_factor"],
                     swap_neighbours=True)
    for k in ("divu", "shear", "vort", "rdg_shear"):
        val, mag = wrong[k]
        out = (np.abs(np.asarray(want["deformations"][k], dtype=R.LD) - val) > R.bound(k, mag))[on]
        assert out.mean() > 0.5, (k, float(out.mean()))
