"""No GPU: the comparisons of tests/test_gpu_call_chain_cgrid.py are not vacuous.  The oracle's chain (tests/evp_cgrid_call_chain.py)
changes its bits at the named stage when the stages after the loop are fed the state of n - 1 subcycles (what a stale allocation is),
when the ghost cells of the final face velocities are zeroed, when strintxE / strintyN go without their halo update, and when call 2
keeps the stresses where the mask lost ice; every stage's output is non-zero on every chain case and the fold rows carry moving ice;
the restatements after the loop reproduce the reference's own arrays on every fixture, tripoleT included (so do the oracle's loop and
preparation there, which the 7- and 8-subcycle calls of those fixtures are compared with); every row of CG_PATHS has a case, and the
calls of every ping-pong row end -- by the host's swap rules restated in predicted_swaps -- in both allocations."""
import numpy as np
import pytest

import evp_cgrid_call_chain as cc
import oracle
from common import CGRID_CASES, CGRID_TFOLD_CASES, GoldenCase, assert_bitwise, bits_equal

AFTER = ("deformations", "dyn_finish", "tail", "dyn_finish_u", "strocn_t")


def differs(a: dict, b: dict):
    return [k for k in a if not bits_equal(a[k], b[k])]


def nonzero(stage: dict):
    return all(np.abs(np.where(v == cc.SENT, 0.0, v)).max() > 0 for v in stage.values())


def test_every_row_has_a_case_and_every_ping_pong_row_ends_in_both_allocations():
    fixture, synth = cc.fixture_rows(), cc.synth_rows()
    assert {p for _, p in fixture + synth} == set(cc.CG_PATHS), set(cc.CG_PATHS) - {p for _, p in fixture + synth}
    for name, path in fixture:
        c = GoldenCase(name)
        counts = [n for _ in range(c.ncalls) for n in c.nsub_list] + list(cc.ODD_EVEN)
        word, seen = 0, cc.Seen(path)
        for n in counts:
            word ^= cc.predicted_swaps(path, n, True)
            seen.add(word)
        seen.assert_both()
    for name, path in synth:
        word, seen = 0, cc.Seen(path)
        for n in [n for pair in cc.PAIRS for n in pair]:
            word ^= cc.predicted_swaps(path, n, True)
            seen.add(word)
        seen.assert_both()
        # ... and the preparation of some call 2 (state = None) reads second allocations
        if path in cc.PING_PONG:      # (the words after the call 1 of each pair: 0 and 2 of the four)
            assert seen.words[0] != 0 or seen.words[2] != 0, path
    # every row has its second call with state = None off the fixtures, where faces gain and lose ice (asserted there)
    assert {p for _, p in synth} == set(cc.CG_PATHS), set(cc.CG_PATHS) - {p for _, p in synth}
    for path in cc.CG_PATHS:
        cc.split_case(path)          # (every row has a case of split calls)
        word, seen = 0, cc.Seen(path)
        for a, b in cc.SPLITS:
            for n, first in ((a, True), (b, False)):
                word ^= cc.predicted_swaps(path, n, first)
                seen.add(word)
        seen.assert_both()


def test_the_fixtures_second_calls_change_the_masks():
    """The three fixtures with two calls (and the tripoleT one): faces gain or lose ice between the calls."""
    two = [n for n in CGRID_CASES + CGRID_TFOLD_CASES if GoldenCase(n).ncalls > 1]
    assert len(two) == 4
    for n in two:
        ch = cc.fixture_masks_change(GoldenCase(n), 2)
        assert {"iceEmask", "iceNmask", "iceTmask"} <= set(ch), (n, ch)


def test_the_seabed_case_has_seabed_stress():
    case = cc.synth_case("closed 100x116 seabed")
    for a, b in case.chain():
        for call in (a, b):
            assert np.abs(call["inputs"]["TbE"]).max() > 0 and np.abs(call["inputs"]["TbN"]).max() > 0
            assert np.abs(call["loop"]["taubxE"]).max() > 0 and np.abs(call["loop"]["taubyN"]).max() > 0


def test_swap_rules_restated():
    """The rules of evp_host_cgrid_loop.cpp as the table has them: the five phases never swap; the three launches swap stress12U alone;
    cg_one / cg_strip swap all five but in the first subcycle after an upload; beside a fold that one runs in place."""
    assert cc.predicted_swaps("five phases", 7, True) == 0 and cc.predicted_swaps("five phases + cg_res FOLD", 7, True) == 0
    assert cc.predicted_swaps("fused, three launches", 7, True) == cc.PP_S12 and cc.predicted_swaps("fused, three launches", 8, False) == 0
    assert cc.predicted_swaps("cg_one", 7, True) == cc.PP_S12 and cc.predicted_swaps("cg_one", 8, True) == cc.PP_FOUR
    assert cc.predicted_swaps("cg_one", 7, False) == cc.PP_ALL and cc.predicted_swaps("cg_one, avg_strength", 8, True) == cc.PP_ALL
    assert cc.predicted_swaps("cg_res", 7, True) == cc.PP_S12 and cc.predicted_swaps("cg_res", 7, False) == 0
    assert cc.predicted_swaps("cg_res", 3, True) == cc.predicted_swaps("cg_one", 3, True)        # (two subcycles left: not resident)
    assert cc.predicted_swaps("marched zone + fold band", 8, True) == cc.PP_ALL and cc.predicted_swaps("marched zone + fold band", 7, True) == 0


@pytest.mark.parametrize("name", CGRID_CASES + CGRID_TFOLD_CASES)
def test_restatements_after_the_loop_reproduce_the_fixtures(name):
    """oracle_post on the reference's final state gives the reference's own divu .. rdg_shear and strocn{x,y}{N,E} on their lists
    and the sentinel elsewhere, and strintxE / strintyN come back from the tail's halo update as the reference left them -- on the
    tripoleT fixtures as well; there the oracle's loop and preparation, which test_oracle_golden.py runs on the other fixtures, equal
    the reference's bit for bit too."""
    c = GoldenCase(name)
    dom = c.oracle_domain()
    for icall in range(1, c.ncalls + 1):
        state, inputs, masks = c.cgrid_inputs(icall)
        uin = cc.u_point_inputs(dom.shape, masks["iceUmask"], seed=17)
        for nsub in c.nsub_list:
            what = f"{name} call {icall} nsub {nsub}"
            want = cc.fixture_want(c, icall, nsub, uin)
            loop = c.cgrid_expected(icall, nsub)
            got = cc.oracle_post(dom, c.oracle_params(), cc.tail_ref.blocks_of(c), c.cgrid_static(), c.d["tarear"], float(c.scal[4]), loop,
                                 inputs, masks, uin)
            for stage in ("deformations", "dyn_finish", "tail", "final"):
                assert_bitwise(got[stage], want[stage], f"{stage}: {what}")
            if name in CGRID_TFOLD_CASES:
                out = oracle.cgrid_subcycle(dom, c.oracle_params(), nsub, state, inputs, c.cgrid_static(), masks, visc_method=str(c.d["visc_method"]))
                oracle.halo_update(dom, out["strintxE"], "Eface", "vector")
                oracle.halo_update(dom, out["strintyN"], "Nface", "vector")
                assert_bitwise(out, loop, f"loop: {what} (the oracle on a T-fold)")
        if name in CGRID_TFOLD_CASES:
            t, st, prev = c.cgrid_prep_inputs(icall)
            got = oracle.cgrid_prep(dom, oracle.PrepParams(**c.prep_scal_dict()), c.cgrid_prep_static(), t, st, prev)
            oracle.halo_update(dom, got["strintxE"], "Eface", "vector")
            oracle.halo_update(dom, got["strintyN"], "Nface", "vector")
            assert_bitwise(got, {k: v for k, v in {**state, **inputs}.items() if k != "strength"}, f"prep: {name} call {icall} (the oracle on a T-fold)")
            assert all(bits_equal(got[k] != 0, masks[k] != 0) for k in oracle.C_MASKS)


@pytest.mark.parametrize("name", CGRID_CASES + CGRID_TFOLD_CASES)
def test_fixture_chain_sees_a_stale_allocation(name):
    c = GoldenCase(name)
    _, inputs, masks = c.cgrid_inputs(c.ncalls)
    uin = cc.u_point_inputs(c.oracle_domain().shape, masks["iceUmask"], seed=17)
    for n in cc.ODD_EVEN:
        good, stale = cc.fixture_oracle_want(c, c.ncalls, n, uin), cc.fixture_oracle_want(c, c.ncalls, n - 1, uin)
        assert differs(good["loop"], stale["loop"]), f"loop + download: {name}: {n - 1} subcycles pass for {n}"
        for stage in AFTER:
            assert differs(good[stage], stale[stage]), f"{stage}: {name}: the state of {n - 1} subcycles passes for {n}"
            assert nonzero(good[stage]), f"{stage}: {name}: all zero"


@pytest.mark.parametrize("name", list(cc.SYNTH))
def test_synthetic_chain_sees_the_planted_errors(name):
    case = cc.synth_case(name)
    last = None
    for (n1, n2), (a, b) in zip(cc.PAIRS, case.chain()):
        case.gains_and_losses(1, a["prep"], case.calls[0]["prev"])
        case.gains_and_losses(2, b["prep"], a["masks"])
        if case.kind in ("fold", "foldT"):
            case.top_rows_move(a["prep"], a["loop"])
            case.top_rows_move(b["prep"], b["loop"])
        for icall, n, good, prev in ((1, n1, a, None), (2, n2, b, a)):
            what = f"{name} call {icall} ndte {n}"
            for stage in AFTER:
                assert nonzero(good[stage]), f"{stage}: {what}: all zero"
            assert all(np.abs(good["loop"][k]).max() > 0 for k in oracle.C_FIELDS[:12]), f"loop: {what}"
            # the stages after the loop fed the state of n - 1 subcycles: a stale allocation
            stale = case.oracle_call(icall, n, prev_call=prev, feed_n=n - 1, last_inputs=last)
            for stage in AFTER + ("final",):
                assert differs(good[stage], stale[stage]), f"{stage}: {what}: the state of {n - 1} subcycles passes for {n}"
            # ghost face velocities zeroed
            ghost = case.oracle_call(icall, n, prev_call=prev, zero_ghost_velocities=True, last_inputs=last)
            assert differs(good["deformations"], ghost["deformations"]), f"deformations: {what}: zeroed ghost velocities pass"
            # strintxE / strintyN without their halo update
            nohalo = case.oracle_call(icall, n, prev_call=prev, tail_halo=False, last_inputs=last)
            assert {"strintxE", "strintyN"} <= set(differs(good["tail"], nohalo["tail"])), f"tail: {what}: a missing halo update passes"
        # call 2 with the stresses kept where the mask lost ice
        kept = case.oracle_prep(2, a, keep_lost_stresses=True)
        assert differs({k: b["prep"][k] for k in cc.PREP_KEYS}, {k: kept[k] for k in cc.PREP_KEYS}), f"prep: {name} call 2: kept stresses pass"
        bad = case.oracle_call(2, n2, prev_call=a, prep=kept)
        assert differs(b["loop"], bad["loop"]), f"loop + download: {name} call 2: stresses kept where the ice went pass"
        last = b["inputs"]


@pytest.mark.parametrize("path", list(cc.CG_PATHS))
def test_split_calls_see_the_state_of_the_first_call(path):
    case = cc.split_case(path)
    for a, b in cc.SPLITS:
        good, _ = cc.split_want(case, a + b)
        stale, _ = cc.split_want(case, a + b, feed_n=a)
        for stage in AFTER:
            assert differs(good[stage], stale[stage]), f"{stage}: {case.name}: the state after subcycle({a}) passes for that after subcycle({b})"
            assert nonzero(good[stage]), f"{stage}: {case.name}: all zero"
