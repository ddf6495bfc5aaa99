"""Cases for the per-call shortcut verdicts ("this operand is redundant on every ice cell: do not read it"): a base state in the
default configuration and deviations of exactly ONE cell each, placed where a classifier is most likely to look past them -- the first
cell of the first block, the last cell of a padded block, a block's east edge, the northernmost ice cell, the only ice cell of a
16 x 16 tile -- and null deviations (the same values where the loop never reads them).  Shared by
tests/test_call_flags_cases_cpu.py (the oracle alone: every real deviation changes its bits, every null one does not -- which is what
makes the GPU comparisons non-vacuous), tests/test_gpu_call_flags.py and tests/test_gpu_cgrid_call_flags.py.

Positions are global 0-based (row, column); a deviation goes into the GLOBAL field before it is scattered, so the ghost images of the
cell carry it too, as they would in the host model.  The ghost-cell and padding-cell nulls go into the block arrays after that."""
from __future__ import annotations

import functools

import numpy as np

from cice_amd import decomp, evp, synth
from test_gpu_parity import run_oracle

NDTE = 7                    # odd: the ping-pong parity flips, the lean loop's two subcycles per trip leave a remainder
B_BLOCKS = (34, 39)         # gx3 (100 x 116) in 3 x 3 blocks, the last column and row of blocks padded (32 columns, 38 rows)
TILE = 16
SCAL = synth.evp_scalars(120)

# kind -> (field, value as a function of the base state's global fields at the cell, the flag the deviation takes away)
B_KINDS = {
    "TbU=0.7": ("TbU", lambda st, p: 0.7, evp.F_TBU_ZERO),
    "TbU=-0.0": ("TbU", lambda st, p: -0.0, evp.F_TBU_ZERO),
    "waterxU+1ulp": ("waterxU", lambda st, p: np.nextafter(st["uocnU"][p], np.inf), evp.F_WATER_IS_OCN),
    "wateryU-1ulp": ("wateryU", lambda st, p: np.nextafter(st["vocnU"][p], -np.inf), evp.F_WATER_IS_OCN),
}
B_POSITIONS = ("first cell of block 0", "last cell of the padded block", "east edge of a block", "northernmost", "alone in its tile")
B_NULLS = ("interior cell without ice", "ghost cell", "padding cell")
B_REAL = [(k, p) for k in B_KINDS for p in B_POSITIONS]


def nearest(cand, j, i, window=None, ok=None):
    """The candidate cell nearest to (j, i), inside the half-open window (j0, j1, i0, i1) if one is given, that satisfies ok(cell) if
    that is given; None if there is none."""
    c = cand.copy()
    if window is not None:
        j0, j1, i0, i1 = window
        keep = np.zeros_like(c)
        keep[j0:j1, i0:i1] = True
        c &= keep
    jj, ii = np.nonzero(c)
    if jj.size == 0:
        return None
    for k in np.argsort((jj - j) ** 2 + (ii - i) ** 2, kind="stable"):
        if ok is None or ok((int(jj[k]), int(ii[k]))):
            return int(jj[k]), int(ii[k])
    return None


def tile_window(b, j, i, ny, nx):
    """The 16 x 16 tile of block b's interior that holds global cell (j, i), as a global window."""
    j0 = b.gj0 - 1 + (j - (b.gj0 - 1)) // TILE * TILE
    i0 = b.gi0 - 1 + (i - (b.gi0 - 1)) // TILE * TILE
    return j0, min(j0 + TILE, b.gj0 - 1 + b.gny, ny), i0, min(i0 + TILE, b.gi0 - 1 + b.gnx, nx)


class BBase:
    """gx3 'caps' (warm), the masks cleared around one ice cell so that it is alone in its 16 x 16 tile (in the 3 x 3 blocks' tiling
    and in the one-block tiling), and the positions of the deviations."""

    def __init__(self):
        spec = synth.GRIDS["gx3"]
        self.nx, self.ny = nx, ny = spec["nx"], spec["ny"]
        self._pos = {}
        self.g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns="closed"))
        self.dcs = {True: decomp.Decomp(nx, ny, *B_BLOCKS, "cyclic", "closed", 1), False: decomp.Decomp(nx, ny, nx, ny, "cyclic", "closed", 1)}
        self.geo = {s: {k: d.scatter(self.g[k], 0, fill=(1.0 if k in ("HTE", "HTN", "dxT", "dyT", "tarea") else 0.0))
                        for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")} for s, d in self.dcs.items()}
        dc = self.dcs[True]
        assert (dc.nblocks_x, dc.nblocks_y) == (3, 3) and dc.blocks[8].gnx < B_BLOCKS[0] and dc.blocks[8].gny < B_BLOCKS[1]
        # the lone cell: an ice U-cell of block 1, in the block's second tile row; everything else of its tile (either tiling) goes.
        # The one nearest to the middle of that tile at which one ulp in waterxU and one in wateryU each survive the oracle's rounding.
        st0 = synth.make_state(self.g, case="caps", seed=20261020, warm=True)
        b1 = dc.blocks[1]
        win = (b1.gj0 - 1 + TILE, b1.gj0 - 1 + 2 * TILE, b1.gi0 - 1, b1.gi0 - 1 + TILE)
        lone = nearest(st0["iceUmask"] != 0, win[0] + 6, win[2] + 7, win, lambda p: self._isolate(st0, p))
        assert lone is not None, "no ice U-cell in the tile chosen for the lone cell where one ulp of water velocity shows"
        self.lone = lone

    def _isolate(self, st0, lone):
        """self.st = st0 with the masks cleared around `lone`; True if both water deviations at `lone` change the oracle's outputs."""
        st = {k: v.copy() for k, v in st0.items()}
        wins = [tile_window(d.blocks[1 if s else 0], *lone, self.ny, self.nx) for s, d in self.dcs.items()]
        for w in wins:
            for k in ("iceTmask", "iceUmask"):
                keep = st[k][lone]
                st[k][w[0]:w[1], w[2]:w[3]] = 0
                st[k][lone] = keep
        for w in wins:
            assert st["iceUmask"][w[0]:w[1], w[2]:w[3]].sum() == 1
        # (dyn_prep2's contract: stresses are zero off the T mask, velocities and the U-cell operands off the U mask)
        for k in evp.FIELDS[:12]:
            st[k] = st[k] * (st["iceTmask"] != 0)
        for k in ("uvel", "vvel", "uvel_init", "vvel_init", "waterxU", "wateryU", "forcexU", "forceyU", "umassdti", "fmU"):
            st[k] = st[k] * (st["iceUmask"] != 0)
        self.st = st
        dc = self.dcs[False]
        base = run_oracle(dc, self.geo[False], *self.inputs(False, ()), SCAL, NDTE)
        return all(differing(run_oracle(dc, self.geo[False], *self.inputs(False, ((kind, lone),)), SCAL, NDTE), base)
                   for kind in ("waterxU+1ulp", "wateryU-1ulp"))

    # the default configuration, asserted: what the shortcuts rest on
    def check_default(self):
        um = self.st["iceUmask"] != 0
        assert um.sum() > 1000
        assert np.array_equal(self.st["waterxU"][um].view(np.uint64), self.st["uocnU"][um].view(np.uint64))
        assert np.array_equal(self.st["wateryU"][um].view(np.uint64), self.st["vocnU"][um].view(np.uint64))
        assert not self.st["TbU"].view(np.uint64).any()
        assert np.array_equal(self.g["tarea"], self.g["dxT"] * self.g["dyT"])

    def positions(self, kind):
        """name -> global (j, i) of an ice U-cell for a deviation of `kind`: one whose undeviated final uvel and vvel are nonzero (so
        that TbU = -0.0 shows in the sign of taubx / tauby there) and, for one ulp in waterxU or wateryU, where that ulp changes the
        oracle's outputs (where the first momentum step rounds it away the deviation is no deviation: the nearest cell where it
        survives is taken)."""
        if kind in self._pos:
            return self._pos[kind]
        dc = self.dcs[False]
        want = b_oracle(False, ())
        u, v = dc.gather({0: want["uvel"]}), dc.gather({0: want["vvel"]})
        cand = (self.st["iceUmask"] != 0) & (u != 0.0) & (v != 0.0)
        blk = self.dcs[True].blocks
        base = b_oracle(False, ())

        def ok(p):
            return bool(differing(run_oracle(dc, self.geo[False], *self.inputs(False, ((kind, p),)), SCAL, NDTE), base))
        win = lambda b: (b.gj0 - 1, b.gj0 - 1 + b.gny, b.gi0 - 1, b.gi0 - 1 + b.gnx)
        b0, b8 = blk[0], blk[8]
        edge = np.zeros_like(cand)                # the last column of blocks 0 and 1: the eastern neighbour is another block
        for b in blk[:2]:
            edge[b.gj0 - 1:b.gj0 - 1 + b.gny, b.gi0 - 1 + b.gnx - 1] = True
        jn = int(np.nonzero(cand.any(axis=1))[0].max())
        pos = {
            "first cell of block 0": nearest(cand, b0.gj0 - 1, b0.gi0 - 1, win(b0), ok),
            "last cell of the padded block": nearest(cand, b8.gj0 - 1 + b8.gny - 1, b8.gi0 - 1 + b8.gnx - 1, win(b8), ok),
            "east edge of a block": nearest(cand & edge, b0.gj0 - 1, b0.gi0 - 1 + b0.gnx - 1, None, ok),
            "northernmost": nearest(cand, jn, self.nx // 2, (jn, jn + 1, 0, self.nx), ok),
            "alone in its tile": self.lone if cand[self.lone] and ok(self.lone) else None,
        }
        for k, p in pos.items():
            assert p is not None, f"no ice U-cell with nonzero final velocity for '{k}'"
        assert len(set(pos.values())) == len(pos), pos
        self._pos[kind] = pos
        return pos

    def null_positions(self):
        """interior: a physical cell without ice, global (j, i); ghost, padding: (block, row, column) of the 3 x 3 blocks' arrays."""
        dc = self.dcs[True]
        off = self.st["iceUmask"] == 0
        um = dc.scatter(self.st["iceUmask"], 0, fill=0)
        b0, b2 = dc.blocks[0], dc.blocks[2]
        rows = np.nonzero(um[b0.local][:, 0])[0]          # the west ghost column of block 0: images across the cyclic boundary
        ghost = (b0.local, int(rows[0]) if rows.size else 1, 0)
        assert b2.gnx < B_BLOCKS[0]
        pad = (b2.local, decomp.NGHOST + 3, decomp.NGHOST + b2.gnx + 1)          # beyond ihi + 1: neither physical nor ghost
        assert pad[2] < dc.nx_block
        inner = nearest(off, self.ny // 2, self.nx // 2)
        assert inner is not None
        return {"interior cell without ice": inner, "ghost cell": ghost, "padding cell": pad}

    def inputs(self, split: bool, devs=()):
        """(fields, iceTmask, iceUmask) as block arrays of the 3 x 3 blocks (split) or of one block, with the deviations applied.
        devs: tuples (kind, position name) -- a real position, or one of B_NULLS."""
        dc = self.dcs[split]
        st = {k: v.copy() for k, v in self.st.items()}
        late = []
        for kind, where in devs:
            field, value, _ = B_KINDS[kind]
            if where in B_POSITIONS or where == "interior cell without ice" or len(where) == 2:
                p = self.positions(kind)[where] if where in B_POSITIONS else (where if len(where) == 2 else self.null_positions()[where])
                st[field][p] = value(self.st, p)
            else:
                assert split, "ghost and padding nulls are defined on the 3 x 3 blocks"
                late.append((field, value, self.null_positions()[where]))
        fields = {k: dc.scatter(st[k], 0) for k in evp.FIELDS}
        for field, value, (b, j, i) in late:
            ocn = {"uocnU": fields["uocnU"][b], "vocnU": fields["vocnU"][b]}
            fields[field][b, j, i] = value(ocn, (j, i))
        return fields, dc.scatter(st["iceTmask"], 0, fill=0), dc.scatter(st["iceUmask"], 0, fill=0)


@functools.lru_cache(maxsize=None)
def b_base() -> BBase:
    return BBase()


@functools.lru_cache(maxsize=None)
def b_inputs(split: bool, devs=()):
    return b_base().inputs(split, devs)


@functools.lru_cache(maxsize=None)
def b_oracle(split: bool, devs=()):
    """The oracle's 18 outputs after NDTE subcycles; computed once per deviation and layout, shared, never written to."""
    base = b_base()
    fields, tm, um = b_inputs(split, devs)
    out = run_oracle(base.dcs[split], base.geo[split], fields, tm, um, SCAL, NDTE)
    for a in out.values():
        a.setflags(write=False)
    return out


def b_cleared(devs) -> int:
    """The flags a set of deviations takes away (real positions only)."""
    m = 0
    for kind, where in devs:
        if where in B_POSITIONS:
            m |= B_KINDS[kind][2]
    return m


def b_pairs():
    """Every real deviation once, as pairs (A, B) for the call sequence default -> A -> default -> B -> A and B -> default: A a seabed
    stress deviation, B a water deviation one position further on, so that the two take different flags away at different cells."""
    n = len(B_POSITIONS)
    kinds = list(B_KINDS)
    return [((kinds[t], B_POSITIONS[q]), (kinds[t + 2], B_POSITIONS[(q + 1) % n])) for t in (0, 1) for q in range(n)]


def differing(a: dict, b: dict):
    """Names of the outputs whose bit patterns differ anywhere."""
    return [k for k in a if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint64), np.ascontiguousarray(b[k]).view(np.uint64))]


# ---- C grid ----------------------------------------------------------------------------------------------------------------------
# The synthetic workload of the marched-kernel tests (tests/test_gpu_cgrid.py: marched_case) at its smallest size, 200 x 48 with holes
# in the four ice masks and islands: as one block (the marched kernel needs the width) and as 3 x 3 blocks of 70 x 20, the last column
# of blocks 60 wide and the last row 8 high.  The flag word of evp_cgrid.hip: cg_call_setup -- a set bit takes the shortcut away.
C_SIZE = (200, 48)
C_BLOCKS = (70, 20)
C_SEED = 21
# kind -> (field, face, value from the base state's global inputs at the cell, the bit the deviation sets)
C_KINDS = {
    "TbE=0.7": ("TbE", "E", lambda inp, p: 0.7, evp.CG_TB_NONZERO),
    "rheofactE=0": ("rheofactE", "E", lambda inp, p: 0.0, evp.CG_RHEOFACT),
    "TbN=0.7": ("TbN", "N", lambda inp, p: 0.7, evp.CG_TB_NONZERO),
    "waterxE+1ulp": ("waterxE", "E", lambda inp, p: np.nextafter(inp["uocnE"][p], np.inf), evp.CG_WATER_DIFFERS),
    "TbE=-0.0": ("TbE", "E", lambda inp, p: -0.0, evp.CG_TB_NONZERO),
    "rheofactN=0.5": ("rheofactN", "N", lambda inp, p: 0.5, evp.CG_RHEOFACT),
    "wateryN-1ulp": ("wateryN", "N", lambda inp, p: np.nextafter(inp["vocnN"][p], -np.inf), evp.CG_WATER_DIFFERS),
}
C_POSITIONS = B_POSITIONS + ("ice on this face only",)
C_NULLS = B_NULLS
C_REAL = [(k, p) for p in C_POSITIONS for k in C_KINDS]


class CBase:
    def __init__(self):
        from test_gpu_cgrid import marched_case_global
        nx, ny = C_SIZE
        self.nx, self.ny = nx, ny
        self._pos = {}
        self.dcs = {True: decomp.Decomp(nx, ny, *C_BLOCKS, "cyclic", "closed", 1), False: decomp.Decomp(nx, ny, nx, ny, "cyclic", "closed", 1)}
        dc = self.dcs[True]
        assert (dc.nblocks_x, dc.nblocks_y) == (3, 3) and dc.blocks[8].gnx < C_BLOCKS[0] and dc.blocks[8].gny < C_BLOCKS[1]
        self.g, self.cg, state0, inputs0, masks0 = marched_case_global(C_SEED, nx, ny, "full", 0.2, 0.02)
        self.prm = oracle_params()
        # the lone cell: ice at both faces, in block 4's first tile; everything else of its tile (either tiling) goes from all four
        # masks.  The one nearest to the middle of the tile where every kind of deviation changes the oracle's outputs.
        b4 = dc.blocks[4]
        win = (b4.gj0 - 1, b4.gj0 - 1 + TILE, b4.gi0 - 1, b4.gi0 - 1 + TILE)
        both = (masks0["iceEmask"] != 0) & (masks0["iceNmask"] != 0)
        lone = nearest(both, win[0] + 7, win[2] + 7, win, lambda p: self._isolate(state0, inputs0, masks0, p))
        assert lone is not None, "no cell in the tile chosen for the lone cell where every deviation shows"
        self.lone = lone

    def _isolate(self, state0, inputs0, masks0, lone):
        masks = {k: v.copy() for k, v in masks0.items()}
        state = {k: v.copy() for k, v in state0.items()}
        wins = [tile_window(d.blocks[4 if s else 0], *lone, self.ny, self.nx) for s, d in self.dcs.items()]
        for w in wins:
            for k in masks:
                keep = masks[k][lone]
                masks[k][w[0]:w[1], w[2]:w[3]] = 0
                masks[k][lone] = keep
        for k in ("stresspT", "stressmT", "stress12T"):
            state[k] = state[k] * masks["iceTmask"]
        state["stress12U"] = state["stress12U"] * masks["iceUmask"]
        self.state, self.inp, self.masks = state, inputs0, masks
        for w in wins:
            assert masks["iceEmask"][w[0]:w[1], w[2]:w[3]].sum() == 1 and masks["iceNmask"][w[0]:w[1], w[2]:w[3]].sum() == 1
        base = self.oracle(False, self.inputs(False, ()))
        return all(differing(self.oracle(False, self.inputs(False, ((kind, lone),))), base) for kind in C_KINDS)

    def check_default(self):
        """The default configuration on every ice face, bit for bit (tests/test_gpu_cgrid.py: the shortcuts' premises)."""
        for t, wat, ocn in (("E", "waterxE", "uocnE"), ("N", "wateryN", "vocnN")):
            on = self.masks[f"ice{t}mask"] != 0
            assert on.sum() > 1000
            assert np.array_equal(self.inp[wat][on].view(np.uint64), self.inp[ocn][on].view(np.uint64))
            assert not self.inp[f"Tb{t}"].view(np.uint64).any() and (self.inp[f"rheofact{t}"][on] == 1.0).all()

    def oracle(self, split, scattered):
        import oracle
        dc = self.dcs[split]
        blks = dc.local_blocks(0)
        dom = oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), dc.nx_global, dc.ny_global, dc.ew, dc.ns,
                                  [b.ilo for b in blks], [b.ihi for b in blks], [b.jlo for b in blks], [b.jhi for b in blks],
                                  [b.gi0 for b in blks], [b.gj0 for b in blks])
        static, state, inputs, masks = scattered
        return oracle.cgrid_subcycle(dom, self.prm, NDTE, state, inputs, static, masks, visc_method="avg_zeta")

    def positions(self, kind):
        """name -> global (j, i) of an ice face of the kind's sort where the deviation changes the oracle's outputs and the undeviated
        final velocity component of that face is nonzero (Tb = -0.0 then shows in the sign of taubx)."""
        if kind in self._pos:
            return self._pos[kind]
        face = C_KINDS[kind][1]
        dc = self.dcs[False]
        base = c_oracle(False, ())
        vel = dc.gather({0: base["uvelE" if face == "E" else "vvelN"]})
        mine, other = self.masks[f"ice{face}mask"] != 0, self.masks[f"ice{'N' if face == 'E' else 'E'}mask"] != 0
        cand = mine & (vel != 0.0)

        def ok(p):
            return bool(differing(self.oracle(False, self.inputs(False, ((kind, p),))), base))
        blk = self.dcs[True].blocks
        win = lambda b: (b.gj0 - 1, b.gj0 - 1 + b.gny, b.gi0 - 1, b.gi0 - 1 + b.gnx)
        b0, b8 = blk[0], blk[8]
        edge = np.zeros_like(cand)
        for b in blk[:2]:
            edge[b.gj0 - 1:b.gj0 - 1 + b.gny, b.gi0 - 1 + b.gnx - 1] = True
        jn = int(np.nonzero(mine.any(axis=1))[0].max())
        pos = {
            "first cell of block 0": nearest(cand, b0.gj0 - 1, b0.gi0 - 1, win(b0), ok),
            "last cell of the padded block": nearest(cand, b8.gj0 - 1 + b8.gny - 1, b8.gi0 - 1 + b8.gnx - 1, win(b8), ok),
            "east edge of a block": nearest(cand & edge, b0.gj0 - 1, b0.gi0 - 1 + b0.gnx - 1, None, ok),
            "northernmost": nearest(cand, jn, self.nx // 2, (jn, jn + 1, 0, self.nx), ok),
            "alone in its tile": self.lone if cand[self.lone] and ok(self.lone) else None,
            "ice on this face only": nearest(cand & ~other, self.ny // 2, self.nx // 2, None, ok),
        }
        for k, p in pos.items():
            assert p is not None, f"{kind}: no ice face for '{k}'"
        assert len(set(pos.values())) == len(pos), pos
        self._pos[kind] = pos
        return pos

    def null_positions(self):
        dc = self.dcs[True]
        none = (self.masks["iceEmask"] == 0) & (self.masks["iceNmask"] == 0)
        em = dc.scatter(self.masks["iceEmask"], 0, fill=0)
        b0, b2 = dc.blocks[0], dc.blocks[2]
        rows = np.nonzero(em[b0.local][:, 0])[0]
        ghost = (b0.local, int(rows[0]) if rows.size else 1, 0)
        pad = (b2.local, decomp.NGHOST + 3, decomp.NGHOST + b2.gnx + 1)
        assert b2.gnx < C_BLOCKS[0] and pad[2] < dc.nx_block
        inner = nearest(none, self.ny // 2, self.nx // 2)
        assert inner is not None
        return {"interior cell without ice": inner, "ghost cell": ghost, "padding cell": pad}

    def inputs(self, split, devs=()):
        """(static, state, inputs, masks) as block arrays with the deviations applied; devs: (kind, position name or global cell)."""
        dc = self.dcs[split]
        inp = {k: v.copy() for k, v in self.inp.items()}
        late = []
        for kind, where in devs:
            field, _, value, _ = C_KINDS[kind]
            if where in C_POSITIONS:
                p = self.positions(kind)[where]
            elif where == "interior cell without ice":
                p = self.null_positions()[where]
            elif where in C_NULLS:
                assert split, "ghost and padding nulls are defined on the 3 x 3 blocks"
                late.append((field, value, self.null_positions()[where]))
                continue
            else:
                p = where
            inp[field][p] = value(self.inp, p)
        static, state, inputs, masks = synth.cgrid_scatter(dc, 0, self.cg, self.state, inp, self.masks)
        for field, value, (b, j, i) in late:
            inputs[field][b, j, i] = value({k: inputs[k][b] for k in ("uocnE", "vocnN")}, (j, i))
        return static, state, inputs, masks


def oracle_params():
    import oracle
    return oracle.make_params(**{k: SCAL[k] for k in ("arlx1i", "denom1", "brlx", "revp", "e_factor", "epp2i", "capping", "Ktens",
                                                      "deltaminEVP", "u0", "cosw", "sinw", "rhow")})


@functools.lru_cache(maxsize=None)
def c_base() -> CBase:
    return CBase()


@functools.lru_cache(maxsize=None)
def c_inputs(split: bool, devs=()):
    return c_base().inputs(split, devs)


@functools.lru_cache(maxsize=None)
def c_oracle(split: bool, devs=()):
    """The oracle's 19 arrays after NDTE subcycles; once per deviation and layout, shared, never written to."""
    out = c_base().oracle(split, c_inputs(split, devs))
    for a in out.values():
        a.setflags(write=False)
    return out


def c_bits(devs) -> int:
    """The bits a set of deviations sets in the C grid's flag word (real positions only)."""
    m = 0
    for kind, where in devs:
        if where in C_POSITIONS:
            m |= C_KINDS[kind][3]
    return m


def c_pairs():
    """Every real deviation once, as pairs (A, B) for the call sequence; the two of a pair are of different kinds."""
    return list(zip(C_REAL[::2], C_REAL[1::2]))
