"""CPU: which schedule the C-grid subcycle loop runs (cice_amd/csrc/cgrid_schedule.cpp: cg_choose_schedule, read through the test
build's cice_evp_hip_debug_cgrid_choose) against the rules restated in numpy from the seven predicates the host used to evaluate one
by one -- each restatement cites the lines of cice_amd/csrc/evp_host_cgrid.cpp as it stood before the chooser existed (the parent of
the commit that added this file).

The product: every boolean fact that some rule combines with another (18 of them, `first` among them), the two tri-state switches,
the resident kernel on or not (res_mode 1; -1 and 0, of which the rules ask nothing but "not 1", take turns) and ndte in
{1, 2, 3, 4, 5, 4001, 4002} -- 2^18 x 9 x 2 x 7 rows, one vectorised call per (tri-states, res_mode, ndte).  Four facts no rule
combines with anything but the chosen kind -- `fast` (copied into the result), the switches MARCH_FOLD_SERIAL and STRIP_LAST and
`synced` (modifiers, gated by the kind) -- do not multiply the product: a hash of the row number spreads their 16 combinations over
the rows, and the test asserts that every kind met every one of them."""
import ctypes as C
import itertools

import numpy as np

from cice_amd import evp

FACTS = ["one_tab", "remote", "tripole", "tfold", "geo", "frame_plan", "one_items", "rest_plan", "rest_items", "by_size", "rest_scr5",
         "avg_strength", "fast", "res_mode", "res_ok", "sw_one", "sw_fused", "sw_march_ranks", "sw_march_fold", "sw_march_fold_ranks",
         "sw_march_avgs", "sw_serial", "sw_strip_last", "ndte", "first", "synced"]          # CgSchedFacts, in order
OUT = ["kind", "nres", "fast", "geo", "serial", "strip_last", "sync"]                       # CgSchedule, in order
PHASES, THREE, ONE, ZONE_FRAME, ZONE_FRAME_PHASES, MARCH_FOLD, MARCH_FOLD_RANKS, PHASES_RESIDENT = range(8)
UNSET = -2 ** 31
PASSED_ON = ["fast", "sw_serial", "sw_strip_last", "synced"]
CROSSED = [k for k in FACTS if k not in PASSED_ON + ["res_mode", "sw_march_fold", "sw_march_fold_ranks", "ndte"]]
NDTE = (1, 2, 3, 4, 5, 4001, 4002)


def choose(lib, rows):
    out = np.empty((len(rows), len(OUT)), np.int32)
    rc = lib.cice_evp_hip_debug_cgrid_choose(C.c_int64(len(rows)), rows.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0
    return dict(zip(OUT, np.ascontiguousarray(out.T)))


def parent_rules(f, b):
    """The parent's predicates, one by one, and its dispatch: what it ran, what it keyed the graph with.  f: the facts, b: as booleans."""
    mf, mfr = f["sw_march_fold"], f["sw_march_fold_ranks"]
    one = b["one_tab"] & ~b["remote"] & b["sw_one"]                                                        # one_launch(): 499
    fused = ~(b["avg_strength"] & ~one) & ~b["tripole"] & b["sw_fused"]                                    # fused_schedule(): 315-320
    march_ranks = (b["frame_plan"] & b["one_items"] & b["remote"] & ~b["tripole"] & ~b["avg_strength"] & b["geo"] &
                   b["sw_one"] & b["sw_march_ranks"])                                                      # march_ranks(): 505-509
    want1 = np.where(~b["sw_one"], 0, np.where(mf != UNSET, (mf != 0).astype(int), 2))                     # march_fold_wanted(): 518-524
    wantr = np.where(~b["sw_one"] | (mf == 0), 0, np.where(mfr != UNSET, (mfr != 0).astype(int), 2))       # march_fold_ranks_wanted(): 531-537
    want = np.where(b["remote"], wantr, want1)                                                             # march_fold_wanted_here(): 538
    march_fold = (b["rest_plan"] & b["one_items"] & b["tripole"] & ~(b["avg_strength"] & ~(b["sw_march_avgs"] & b["rest_scr5"])) &
                  ((want == 1) | ((want == 2) & b["by_size"])))                                            # march_fold(): 539-547
    frame_phases = (b["rest_plan"] & b["rest_items"] & ~b["tripole"] & b["remote"] & b["avg_strength"] & b["geo"] &
                    b["sw_march_avgs"] & b["sw_one"] & b["sw_march_ranks"])                                # march_frame_phases(): 552-556
    eligible = np.where(b["tripole"], ~(b["tfold"] | b["remote"]), b["one_tab"] & ~b["remote"] & fused & one) & b["res_ok"]   # res_eligible(): 1207-1226
    n = f["ndte"] - b["first"]
    res_sub = np.where((f["res_mode"] == 1) & (b["tripole"] | one) & eligible & (n >= 3) & (n <= 4000), n, 0)   # res_subcycles(): 1327-1332
    # cice_evp_hip_cgrid_subcycle: 1576-1597
    nres = np.where(fused | b["tripole"], res_sub, 0)
    mfold = (nres == 0) & (march_fold | frame_phases)
    key = dict(fused=fused, one=fused & one, march=fused & march_ranks, mfold=mfold, mfold_serial=mfold & b["sw_serial"],
               mfold_sync=mfold & ~b["first"] & ~b["synced"], mfold_ranks=mfold & b["remote"], fast=b["fast"], geo=b["geo"])
    # what the dispatch lambda (1583-1588), enqueue_fused (654, 670, 694) and enqueue_march_fold's counters (642-643) made of them,
    # each kind stated on its own
    ran = np.stack([~fused & (nres == 0) & ~mfold,                                   # five phases
                    fused & ~one & ~march_ranks,                                      # three fused launches
                    fused & one,                                                      # cg_one
                    fused & ~one & march_ranks,                                       # zone marched + frame
                    ~fused & (nres == 0) & mfold & ~b["tripole"],                     # ... on the five phases
                    ~fused & (nres == 0) & mfold & b["tripole"] & ~b["remote"],       # marched zone + fold band
                    ~fused & (nres == 0) & mfold & b["tripole"] & b["remote"],        # ... + frame
                    ~fused & (nres > 0)])                                             # five phases + cg_res FOLD
    return dict(one=one, fused=fused, nres=nres, mfold=mfold, mfold_raw=march_fold | frame_phases, key=key, ran=ran,
                strip_last=b["sw_strip_last"])

def test_chooser_against_the_parents_predicates():
    lib = evp.load_library(testing=True)
    n = 1 << len(CROSSED)
    idx = np.arange(n, dtype=np.int64)
    rows = np.zeros((n, len(FACTS)), np.int32)         # what the library reads, and the same by columns
    col = {k: i for i, k in enumerate(FACTS)}
    f = {k: np.zeros(n, np.int32) for k in FACTS}
    for bit, k in enumerate(CROSSED):
        f[k][:] = idx >> bit & 1
    for bit, k in enumerate(PASSED_ON):
        f[k][:] = (idx * 0x9E3779B1 >> 40) >> bit & 1         # (a hash of the row number: lines up with no crossed bit)
    for k in CROSSED + PASSED_ON:
        rows[:, col[k]] = f[k]
    b = {k: f[k] != 0 for k in CROSSED + PASSED_ON}
    passed = f["fast"] | f["sw_serial"] << 1 | f["sw_strip_last"] << 2 | f["synced"] << 3
    fold9 = f["tripole"] << 9
    kinds_seen, combos_seen, keys, modes_off = set(), set(), {}, itertools.cycle((-1, 0))
    for mf, mfr, on, ndte in itertools.product((UNSET, 0, 1), (UNSET, 0, 1), (True, False), NDTE):
        mode = 1 if on else next(modes_off)
        for k, v in (("sw_march_fold", mf), ("sw_march_fold_ranks", mfr), ("res_mode", mode), ("ndte", ndte)):
            if f[k][0] != v:
                f[k][:] = v
                rows[:, col[k]] = v
        got, want = choose(lib, rows), parent_rules(f, b)
        where = lambda bad: (mf, mfr, mode, ndte, {k: int(f[k][bad[0]]) for k in FACTS}, {k: int(got[k][bad[0]]) for k in OUT})
        # exactly one kind per row, and it is the chooser's; what the parent held by argument: a fused schedule never meets a marched
        # split one on the five phases
        ran = want["ran"].view(np.uint8)
        assert (ran.sum(axis=0, dtype=np.uint8) == 1).all()
        assert not (want["fused"] & want["mfold_raw"]).any()
        bad = np.flatnonzero((ran * np.arange(8, dtype=np.uint8)[:, None]).sum(axis=0, dtype=np.uint8) != got["kind"])
        assert bad.size == 0, where(bad)
        bad = np.flatnonzero(want["nres"] != got["nres"])
        assert bad.size == 0, where(bad)
        # cg_res rides on the one-launch schedule or on a fold, nowhere else
        kind, nres = got["kind"], got["nres"]
        assert np.isin(kind[nres > 0], (ONE, PHASES_RESIDENT)).all() and not ((kind == THREE) & want["one"]).any()
        assert ((kind == PHASES_RESIDENT) <= (nres > 0)).all()
        # the modifiers: fast and geo of every call, the others 0 wherever the kind does not read them
        marched = (kind == ZONE_FRAME_PHASES) | (kind == MARCH_FOLD) | (kind == MARCH_FOLD_RANKS)
        k = want["key"]
        for name, val in (("fast", k["fast"]), ("geo", k["geo"]), ("serial", k["mfold_serial"]), ("sync", k["mfold_sync"]),
                          ("strip_last", (marched | (kind == ONE)) & want["strip_last"])):
            bad = np.flatnonzero(got[name] != val)
            assert bad.size == 0, (name, where(bad))
        assert not got["serial"][~marched].any() and not got["sync"][~marched].any()
        # the graph key (calls with nres == 0): the parent's booleans are functions of the schedule, and the schedule -- STRIP_LAST
        # apart, which the parent baked into a graph without keying it -- is a function of the parent's booleans and the fold, which
        # no call changes: calls that had different keys still have, calls that shared a graph still share it
        old = np.packbits(np.stack([k[name] for name in ("fused", "one", "march", "mfold", "mfold_serial", "mfold_sync", "mfold_ranks", "fast")]),
                          axis=0, bitorder="little")[0].astype(np.int32) | k["geo"].astype(np.int32) << 8 | fold9
        new = kind | got["fast"] << 4 | got["geo"] << 5 | got["serial"] << 6 | got["sync"] << 7
        for code in np.flatnonzero(np.bincount((old << 8 | new)[nres == 0])).tolist():
            o, w = code >> 8, code & 255
            assert keys.setdefault(("old, fold", o), w) == w and keys.setdefault(("new", w), o & 511) == o & 511, (hex(o), hex(w))
        kinds_seen |= set(np.flatnonzero(np.bincount(kind)).tolist())
        combos_seen |= set(np.flatnonzero(np.bincount(kind * 16 + passed)).tolist())
    assert kinds_seen == set(range(8))
    assert len(combos_seen) == 8 * 16          # every kind met every combination of the four facts that are passed on
