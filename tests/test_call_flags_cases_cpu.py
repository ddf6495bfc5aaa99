"""CPU: the make-up of the cases tests/test_gpu_call_flags.py and tests/test_gpu_cgrid_call_flags.py run on the GPU
(tests/call_flag_cases.py).  The oracle alone: every one-cell deviation changes the bits of its outputs -- so a kernel that kept its
shortcut would be caught --, every null deviation leaves them as they were, and the positions are the ones the cases are named for."""
import numpy as np
import pytest

import call_flag_cases as cf
from cice_amd import decomp


def test_bgrid_base_state_and_positions():
    base = cf.b_base()
    base.check_default()
    dc = base.dcs[True]
    um = base.st["iceUmask"] != 0
    blk = dc.blocks
    owner = lambda p: next(b.gid for b in blk if b.gj0 - 1 <= p[0] < b.gj0 - 1 + b.gny and b.gi0 - 1 <= p[1] < b.gi0 - 1 + b.gnx)
    want = cf.b_oracle(False, ())
    u, v = base.dcs[False].gather({0: want["uvel"]}), base.dcs[False].gather({0: want["vvel"]})
    assert np.abs(u).max() > 1e-3                             # the undeviated call moves ice
    for kind in cf.B_KINDS:
        pos = base.positions(kind)
        print(kind, pos)
        for p in pos.values():
            assert um[p] and u[p] != 0.0 and v[p] != 0.0      # ... and the final velocity at every position is nonzero in both components
        assert owner(pos["first cell of block 0"]) == 0 and owner(pos["last cell of the padded block"]) == 8
        e = pos["east edge of a block"]
        assert owner(e) in (0, 1) and e[1] == blk[owner(e)].gi0 - 1 + cf.B_BLOCKS[0] - 1
        assert pos["northernmost"][0] == np.nonzero(um.any(axis=1))[0].max()
        assert pos["alone in its tile"] == base.lone
    for d in base.dcs.values():          # alone in its tile under both tilings
        b = next(b for b in d.blocks if b.gj0 - 1 <= base.lone[0] < b.gj0 - 1 + b.gny and b.gi0 - 1 <= base.lone[1] < b.gi0 - 1 + b.gnx)
        w = cf.tile_window(b, *base.lone, base.ny, base.nx)
        assert um[w[0]:w[1], w[2]:w[3]].sum() == 1 and (w[1] - w[0]) * (w[3] - w[2]) > 1
    nul = base.null_positions()
    assert not um[nul["interior cell without ice"]]
    b, j, i = nul["ghost cell"]
    assert i == 0                                             # a ghost column
    b, j, i = nul["padding cell"]
    assert i > decomp.NGHOST + blk[2].gnx and decomp.NGHOST <= j < decomp.NGHOST + blk[2].gny


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("kind,where", cf.B_REAL)
def test_bgrid_real_deviation_changes_the_oracle(kind, where, split):
    base = cf.b_base()
    want0, want = cf.b_oracle(split, ()), cf.b_oracle(split, ((kind, where),))
    diff = cf.differing(want, want0)
    assert diff, f"{kind} at {where}: the oracle's 18 outputs are unchanged"
    if kind == "TbU=-0.0":
        # Cb = -0.0 enters every sum as nothing; taubx = -uvel * Cb takes the other sign of zero at that one cell
        assert set(diff) == {"taubxU", "taubyU"}, diff
        dc = base.dcs[split]
        p = base.positions(kind)[where]
        for k in ("taubxU", "taubyU"):
            a, b = dc.gather({0: want[k]}), dc.gather({0: want0[k]})
            assert a[p] == 0.0 and b[p] == 0.0 and np.signbit(a[p]) != np.signbit(b[p])
            a, b = a.copy(), b.copy()
            a[p] = b[p] = 0.0
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("where", cf.B_NULLS)
def test_bgrid_null_deviation_leaves_the_oracle_alone(where):
    devs = tuple((k, where) for k in cf.B_KINDS)
    f0, f1 = cf.b_inputs(True, ())[0], cf.b_inputs(True, devs)[0]
    assert sorted(cf.differing(f1, f0)) == ["TbU", "waterxU", "wateryU"]            # the deviation is there
    assert not cf.differing(cf.b_oracle(True, devs), cf.b_oracle(True, ()))


def test_bgrid_pairs_cover_every_real_deviation():
    seen = [d for pair in cf.b_pairs() for d in pair]
    assert sorted(seen) == sorted(cf.B_REAL)
    for a, b in cf.b_pairs():
        want = cf.b_oracle(True, (a, b))
        assert cf.differing(want, cf.b_oracle(True, (a,))) and cf.differing(want, cf.b_oracle(True, (b,)))


def test_cgrid_base_state_and_positions():
    base = cf.c_base()
    base.check_default()
    blk = base.dcs[True].blocks
    owner = lambda p: next(b.gid for b in blk if b.gj0 - 1 <= p[0] < b.gj0 - 1 + b.gny and b.gi0 - 1 <= p[1] < b.gi0 - 1 + b.gnx)
    want = cf.c_oracle(False, ())
    assert np.abs(want["uvelE"]).max() > 1e-3
    for kind, (field, face, _, _) in cf.C_KINDS.items():
        pos = base.positions(kind)
        print(kind, pos)
        mine, other = base.masks[f"ice{face}mask"] != 0, base.masks[f"ice{'N' if face == 'E' else 'E'}mask"] != 0
        vel = base.dcs[False].gather({0: want["uvelE" if face == "E" else "vvelN"]})
        for p in pos.values():
            assert mine[p] and vel[p] != 0.0
        assert owner(pos["first cell of block 0"]) == 0 and owner(pos["last cell of the padded block"]) == 8
        e = pos["east edge of a block"]
        assert owner(e) in (0, 1) and e[1] == blk[owner(e)].gi0 - 1 + cf.C_BLOCKS[0] - 1
        assert pos["northernmost"][0] == np.nonzero(mine.any(axis=1))[0].max()
        assert pos["alone in its tile"] == base.lone and not other[pos["ice on this face only"]]
    for s, d in base.dcs.items():
        w = cf.tile_window(d.blocks[4 if s else 0], *base.lone, base.ny, base.nx)
        for k in ("iceEmask", "iceNmask"):
            assert base.masks[k][w[0]:w[1], w[2]:w[3]].sum() == 1
    nul = base.null_positions()
    assert not base.masks["iceEmask"][nul["interior cell without ice"]] and not base.masks["iceNmask"][nul["interior cell without ice"]]
    assert nul["ghost cell"][2] == 0 and nul["padding cell"][2] > decomp.NGHOST + blk[2].gnx


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("kind,where", cf.C_REAL)
def test_cgrid_real_deviation_changes_the_oracle(kind, where, split):
    base = cf.c_base()
    want0, want = cf.c_oracle(split, ()), cf.c_oracle(split, ((kind, where),))
    diff = cf.differing(want, want0)
    assert diff, f"{kind} at {where}: the oracle's 19 arrays are unchanged"
    if kind == "TbE=-0.0":
        assert diff == ["taubxE"], diff
        p = base.positions(kind)[where]
        a, b = base.dcs[split].gather({0: want["taubxE"]}), base.dcs[split].gather({0: want0["taubxE"]})
        assert a[p] == 0.0 and b[p] == 0.0 and np.signbit(a[p]) != np.signbit(b[p])


@pytest.mark.parametrize("where", cf.C_NULLS)
def test_cgrid_null_deviation_leaves_the_oracle_alone(where):
    devs = tuple((k, where) for k in cf.C_KINDS)
    f0, f1 = cf.c_inputs(True, ())[2], cf.c_inputs(True, devs)[2]
    # (the deviation is there; on a padding cell rheofact = 0 is what the array holds anyway)
    assert {"TbE", "TbN", "rheofactN"} <= set(cf.differing(f1, f0)) <= {"TbE", "TbN", "rheofactE", "rheofactN", "waterxE", "wateryN"}
    assert not cf.differing(cf.c_oracle(True, devs), cf.c_oracle(True, ()))


def test_cgrid_pairs_cover_every_real_deviation():
    pairs = cf.c_pairs()
    assert sorted(d for pair in pairs for d in pair) == sorted(cf.C_REAL)
    for a, b in pairs:
        assert a[0] != b[0]
        assert cf.differing(cf.c_oracle(True, (a, b)), cf.c_oracle(True, ()))
