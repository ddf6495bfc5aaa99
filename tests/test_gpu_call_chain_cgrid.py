"""GPU (-m gpu), one rank: a whole evp() call on the C grid -- cgrid_prep (the state handed in, then None), cgrid_set_tb,
cgrid_prep_finish, the loop, cgrid_download, cgrid_deformations, cgrid_dyn_finish, cgrid_tail, cgrid_dyn_finish_u, cgrid_strocn_t and
cgrid_download again -- behind EVERY schedule of the loop (tests/evp_cgrid_call_chain.py: CG_PATHS): cg_one, the three fused launches,
the five phases, cg_strip with and without its LAST instantiation, cg_res (several blocks, one block, SLOW, the FOLD variant behind the
five phases), the marched zone + fold band on tripole and tripoleT grids and in the serial order, avg_strength wherever it is accepted.
The loop alone is pinned per schedule elsewhere; here it is the hand-over that is under test: the allocation each of uvelE, vvelN,
stresspT, stressmT and stress12U ends in (CG.f[...] after Ran::swapped), which every call after the loop and the next cgrid_prep
without a state read.  Every stage against the reference's own arrays where a fixture holds them and against the oracle's chain
elsewhere, bit for bit on every cell, the stage named in every message; every call asserts that its schedule ran and that in_alt
moved as that schedule's swaps say (assert_cg_path_ran), every test that its ping-pong row ended in both allocations (Seen).
tests/test_cgrid_call_chain_cpu.py shows without a GPU that these comparisons see a stale allocation, a zeroed ghost cell, a missing
halo update and stresses kept where the ice went."""
import numpy as np
import pytest

import evp_cgrid_call_chain as cc
from common import GoldenCase

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,path", cc.fixture_rows())
def test_fixture_chain_on_every_schedule(name, path, monkeypatch):
    """Every call and count of the fixture on ONE core as consecutive evp() calls against the reference's arrays (the second call's
    first run with state = None), then 7 and 8 subcycles through the oracle's chain."""
    cc.set_cg_path(monkeypatch, path)
    c = GoldenCase(name)
    core = cc.fixture_core(c)
    try:
        seen = cc.run_fixture_chain(core, c, path)
        print(f"{name} on {path}: in_alt after each call {[hex(w) for w in seen.words]}")
    finally:
        core.finalize()


PAIRS = cc.PAIRS


def five_phase_loops(case, monkeypatch):
    """tripoleT: the downloads of the same calls on the five-phase schedule, which the tripoleT fixtures pin on the reference."""
    cc.set_cg_path(monkeypatch, "five phases")
    core = case.open_core()
    out = {}
    try:
        for (n1, n2), (a, b) in zip(PAIRS, case.chain()):
            seen, prev = cc.Seen("five phases"), None
            for icall, n, want in ((1, n1, a), (2, n2, b)):
                out[(n1, n2, icall)], prev = cc.run_synth_call(core, case, icall, n, "five phases", want, seen, prev)
    finally:
        core.finalize()
    return out


@pytest.mark.parametrize("name,path", cc.synth_rows())
def test_two_calls_where_faces_gain_and_lose_ice(name, path, monkeypatch):
    """Off the fixtures, behind EVERY row of the table -- the marched schedules on the smallest grids at which a zone forms, the
    fixture-sized ones on a gx3-sized closed grid and a tx3-sized u-fold grid --: call 1 from a state handed in, call 2 with state = None and
    T-grid fields of another seed -- faces gain and lose ice, asserted --, the oracle's chain fed its own call-1 outputs.  What it
    catches: a second allocation left stale where ice vanished, a preparation that read the wrong allocation, a graph keyed on the
    wrong in_alt.  On the fold grids the ice moves on the top three rows."""
    case = cc.synth_case(name)
    ref = five_phase_loops(case, monkeypatch) if case.kind == "foldT" else {}
    cc.set_cg_path(monkeypatch, path)
    core = case.open_core()
    seen = cc.Seen(path)
    try:
        for (n1, n2), (a, b) in zip(PAIRS, case.chain()):
            if case.kind in ("fold", "foldT"):
                case.top_rows_move(b["prep"], b["loop"])
            prev = None
            for icall, n, want in ((1, n1, a), (2, n2, b)):
                _, prev = cc.run_synth_call(core, case, icall, n, path, want, seen, prev, reference=ref.get((n1, n2, icall)))
        print(f"{name} on {path}: in_alt after each call {[hex(w) for w in seen.words]}")
        seen.assert_both()
    finally:
        core.finalize()


@pytest.mark.parametrize("path", list(cc.CG_PATHS))
def test_split_subcycle_calls_then_the_calls_after_the_loop(path, monkeypatch):
    """upload, subcycle(3), subcycle(4), and once more 4 + 3: the calls after the loop must see the state of the second call."""
    cc.set_cg_path(monkeypatch, path)
    case = cc.split_case(path)
    core = case.open_core()
    seen = cc.Seen(path)
    try:
        for a, b in cc.SPLITS:
            want = cc.run_split_calls(core, case, path, seen, a, b)
        assert np.abs(want["loop"]["uvelE"] - case.state["uvelE"]).max() > 0
        seen.assert_both()
        print(f"{case.name} on {path}: in_alt after each call {[hex(w) for w in seen.words]}")
    finally:
        core.finalize()
