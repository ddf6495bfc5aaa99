"""CPU: the marching path on a tripole / tripoleT grid split over several ranks, as every rank plans it from the global block table
through the host-only entry cice_evp_hip_march_layout (cice_amd/csrc/march_plan.cpp: build_march_layout).

One zone (global rows 0 .. zone-1, marched in every rank's strip-major rectangle) and one fold band (rows zone .. NY-1, one subcycle
per launch in the block layout of the ranks whose blocks reach above the zone).  A rank's rectangle is its blocks cut off at row
`zone`; a top rank's northern neighbour is its own columns of the band, so the ext + P columns it holds beyond its own go on above
the zone, where they are rows of its x-neighbour's band: the corner cells, which travel with the rank ring.

The rule all sides live by (tests/test_march_fold_plan_cpu.py): a subcycle computes a cell from the 3 x 3 cells around it in the
state before, so whoever advances a set of cells from a state that is current on a set loses one cell per subcycle at every edge
that is not a boundary; exchanges copy cells that are current where they are owned to where they are only read."""
import numpy as np
import pytest

from cice_amd import decomp, evp

P = 4                      # EVP_MARCH_PAD
SHAPES = ((2, 1), (1, 2), (2, 2), (3, 1))
GRIDS = ((120, 80), (97, 61))
FOLDS = ("tripole", "tripoleT")
EXTS = (0, 4, 8)


def drop(dc, dropped):
    """dc with the blocks at the (iblock, jblock) positions `dropped` eliminated (land), local indices renumbered"""
    for b in dc.blocks:
        if (b.iblock, b.jblock) in dropped:
            b.owner = -1
    for r in range(dc.nranks):
        for k, b in enumerate(sorted((b for b in dc.blocks if b.owner == r), key=lambda b: b.gid)):
            b.local = k
    return dc


def layout_of(nx, ny, ns, shape, blocks_per_rank=(1, 1)):
    world = shape[0] * shape[1]
    dc = decomp.per_rank_blocks(nx, ny, world, "cyclic", ns, proc_shape=shape)
    if blocks_per_rank != (1, 1):
        sx, sy = blocks_per_rank
        dc = decomp.Decomp(nx, ny, -(-dc.block_size_x // sx), -(-dc.block_size_y // sy), "cyclic", ns, world, dc.proc_shape)
    return dc


def plan_all(dc, **ask):
    out, keep = [], []
    for r in range(dc.nranks):
        d, k = evp.make_dims(dc, r)
        keep.append(k)
        out.append(evp.march_layout(d, **ask))
    return out


def owner_map(dc):
    own = np.full((dc.ny_global, dc.nx_global), -1)
    for b in dc.blocks:
        own[b.gj0 - 1:b.gj0 - 1 + b.gny, b.gi0 - 1:b.gi0 - 1 + b.gnx] = b.owner
    return own


def cells_of(L, pos, nx):
    """positions of a rank's strip-major buffers -> global (row, column) of the cells (column wrapped: the grids are cyclic in x)"""
    pos = np.asarray(pos, dtype=np.int64)
    blk, lane = pos >> 6, pos & 63
    row, strip = blk // L["nstrips"], blk % L["nstrips"]
    x = strip * L["own"] + lane - P
    y = row - P
    return L["gy0"] + y, (L["gx0"] + x) % nx


def expected_recv(dc, own, Ls, D):
    """The cells rank D receives, restated: every cell of what D holds (its own cut off at row `zone`, ext more on every side with a
    neighbour) and of the P-cell ring around that, which D does not own and which is a cell of the grid -- but not the rows above
    the zone over D's own columns, which D gathers from its own band.  Owner: the uncut table (a cell above the zone belongs to the
    band of the top rank over it).  Order: rows, then columns, of D's rectangle; peers by ascending rank."""
    nx, ny = dc.nx_global, dc.ny_global
    L = Ls[D]
    zone, ext = L["fold_zone"], L["ext"]
    oy, ox = np.nonzero(own == D)
    gx0, gx1, gy0 = ox.min(), ox.max() + 1, oy.min()
    gy1 = min(oy.max() + 1, zone)
    spans = gx1 - gx0 == nx                                  # wraps inside: no neighbour in x
    w = e = 0 if spans else ext
    s = ext if gy0 > 0 else 0
    n = ext                                                  # a rank above, or the band
    out = []
    for gy in range(gy0 - s - P, gy1 + n + P):
        if gy < 0 or gy >= ny:
            continue
        for x in range(gx0 - w - P, gx1 + e + P):
            own_col = gx0 <= x < gx1
            if own_col and gy0 <= gy < gy1:
                continue
            if gy >= zone and own_col:
                continue
            if spans and not 0 <= x < nx:
                continue
            src = own[gy, x % nx]
            assert src >= 0
            out.append((int(src), gy, x % nx))
    return out


def split_by_peer(L, which):
    cut = L["cut_send" if which == "send" else "cut_recv"]
    pos = L["send_pos" if which == "send" else "recv_pos1"]
    return {int(r): pos[cut[q]:cut[q + 1]] for q, r in enumerate(L["peer_rank"])}


def check_lists(dc, Ls):
    nx = dc.nx_global
    own = owner_map(dc)
    zone = Ls[0]["fold_zone"]
    corners = 0
    recv = [split_by_peer(L, "recv") for L in Ls]
    send = [split_by_peer(L, "send") for L in Ls]
    for D, L in enumerate(Ls):
        want = expected_recv(dc, own, Ls, D)
        assert sorted({w[0] for w in want}) == sorted(recv[D]), (D, sorted(recv[D]))
        for S in recv[D]:
            ws = [(gy, gx) for src, gy, gx in want if src == S]
            gy, gx = cells_of(L, recv[D][S], nx)
            assert ws == list(zip(gy.tolist(), gx.tolist())), f"rank {D} <- {S}: the receive list is not the restated set, in its order"
            # ... and S sends exactly these cells, in this order, from positions of ITS rectangle (rows above the zone among them)
            sy, sx = cells_of(Ls[S], send[S][D], nx)
            assert ws == list(zip(sy.tolist(), sx.tolist())), f"rank {S} -> {D}: the send list does not match the receiver's, cell by cell"
            assert (np.asarray(send[S][D]) >> 6).max() // Ls[S]["nstrips"] < Ls[S]["rows"]
            corners += sum(1 for y, _ in ws if y >= zone)
            assert all(own[y, x] == S for y, x in ws)
    return corners


def simulate(dc, Ls, ndte, kpass, ring_last=False):
    """Every rank over ndte subcycles with the host's schedule and step order (evp_host_march.cpp: march_run): pass; band subcycles,
    each with the velocity halo on every rank; at a trade, on the ranks that hold both: band rows into the rectangle, then the rank
    ring (the layout's own lists), then zone rows into the block layout.  Arrays over the global grid per rank: is what the rank holds
    for that cell current -- in its rectangle (Z: all 14 fields of a cell), in its block layout the velocities (U: interior and
    ghost cells) and the stresses (T: interior and the east / north fringe each block computes for itself and carries from one
    subcycle to the next; no halo touches them)?  A subcycle: a T-cell's stresses from their old values and the velocities at its
    four corners, a U-cell's velocity from its old value and the stresses of the four T-cells around it.
    ring_last: the order that does NOT work -- both halves of the trade, a velocity halo, then the ring.  None, or what went wrong."""
    nx, ny = dc.nx_global, dc.ny_global
    own = owner_map(dc)
    L0 = Ls[0]
    zone, ext, row0 = L0["fold_zone"], L0["ext"], L0["list_row0"]
    ring = ext + P
    R = range(dc.nranks)
    rowsel = lambda lo, hi: (np.arange(ny) >= lo)[:, None] & (np.arange(ny) < hi)[:, None] & np.ones((1, nx), bool)
    tb, tr = rowsel(zone - ring, zone), rowsel(zone, zone + ring)

    def at(v, dy, dx, beyond):
        """v at (row + dy, column + dx): columns cyclic, rows outside the grid = beyond"""
        w = np.roll(v, -dx, 1)
        out = np.full_like(w, beyond)
        if dy == 0:
            return w
        if dy > 0:
            out[:-dy] = w[dy:]
        else:
            out[-dy:] = w[:dy]
        return out

    def grow(m, k):
        """cells within k (Chebyshev) of a cell of m"""
        out = m.copy()
        for _ in range(k):
            out = np.logical_or.reduce([at(out, dy, dx, False) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
        return out

    interior = [own == r for r in R]
    ghost = [grow(interior[r], 1) & ~interior[r] for r in R]
    fringe = [(at(interior[r], 0, -1, False) | at(interior[r], -1, 0, False) | at(interior[r], -1, -1, False)) & ~interior[r] for r in R]
    own_zone = [interior[r] & rowsel(0, zone) for r in R]
    own_band = [interior[r] & rowsel(zone, ny) for r in R]
    band = [bool(own_band[r].any()) for r in R]
    adv, store = [], []
    for r in R:
        L = Ls[r]
        m = np.zeros((ny, nx), bool)
        ys = np.arange(L["gy0"], L["gy0"] + L["nyr"])
        xs = np.arange(L["gx0"], L["gx0"] + L["nxr"]) % nx
        m[np.ix_(ys[(ys >= 0) & (ys < ny)], xs)] = True
        adv.append(m)                                       # the cells a pass advances: own + rim
        store.append(grow(m, P))                            # ... and the P-cell ring it reads
        assert L["nxr"] + 2 * P <= nx or L["wrapx"], "the rectangle would overlap itself on this grid"
    Z = [store[r].copy() for r in R]                        # the gather and the exchanges at the start of a call
    U = [interior[r] | ghost[r] for r in R]
    T = [interior[r] | fringe[r] for r in R]

    def halo():
        src = np.zeros((ny, nx), bool)
        for r in R:
            src |= U[r] & interior[r]
        for r in R:
            U[r] = (U[r] & interior[r]) | (src & ghost[r])

    recv = [split_by_peer(L, "recv") for L in Ls]
    cells = [{S: cells_of(Ls[D], recv[D][S], nx) for S in recv[D]} for D in R]

    def ring_exchange():
        before = [z.copy() for z in Z]
        for D in R:
            for S, (gy, gx) in cells[D].items():
                if not store[S][gy, gx].all():
                    return f"rank {S} is asked for a cell its rectangle does not hold"
                Z[D][gy, gx] = before[S][gy, gx]
        return None

    def to_rect(r):
        src = U[r] & T[r]
        if not (src | ~(tr & interior[r])).all():
            return f"rank {r}: the trade copied a stale row of the block layout into the rectangle"
        Z[r] = np.where(tr & store[r], src, Z[r])

    def to_block(r, rows):
        if not (Z[r] | ~(rows & interior[r])).all():
            return f"rank {r}: a stale row of the rectangle went into the block layout"
        U[r] = np.where((interior[r] | ghost[r]) & rows & store[r], Z[r], U[r])
        T[r] = np.where((interior[r] | fringe[r]) & rows & store[r], Z[r], T[r])

    for k, exch, fexch, last in evp.march_schedule(ndte, kpass, ring, True, True):
        if k == 1:                                 # (a single left-over subcycle runs first, over the whole domain, in the block layout)
            continue
        for r in R:
            # (the closed south edge: nothing beyond it is read; beyond the top of what is stored: nothing valid)
            v = np.vstack([np.ones((k, nx), bool), Z[r], np.zeros((k, nx), bool)])
            Z[r] = ~grow(~v, k)[k:-k] & adv[r]
            if not (Z[r] | ~own_zone[r]).all():
                return f"rank {r}: a pass of {k} read a stale cell for a zone cell it owns"
        for _ in range(k):
            for r in R:
                if not band[r]:                    # (launches nothing: what its block layout holds is a state older)
                    U[r], T[r] = np.zeros((ny, nx), bool), np.zeros((ny, nx), bool)
                    continue
                lst = rowsel(row0, ny)
                # (beyond the fold: the ghost row, which the halo step and the fold logic keep current)
                t = (interior[r] | fringe[r]) & lst & T[r] & U[r] & at(U[r], 0, -1, True) & at(U[r], -1, 0, True) & at(U[r], -1, -1, True)
                u = interior[r] & lst & U[r] & t & at(t, 0, 1, True) & at(t, 1, 0, True) & at(t, 1, 1, True)
                U[r], T[r] = u, t
                if not ((u & t) | ~own_band[r]).all():
                    return f"rank {r}: a band subcycle read a stale cell for a band cell it owns"
            halo()
        steps = []
        if fexch:
            steps = [(to_rect,), (to_block, tb), (halo,), (ring_exchange,)] if ring_last else [(to_rect,), (ring_exchange,), (to_block, tb)]
        elif exch:
            steps = [(ring_exchange,)]
        if fexch and not exch:
            return "zone and band traded rows but the rank ring did not travel"
        for f, *arg in steps:
            for bad in ([f()] if f in (halo, ring_exchange) else [f(r, *arg) for r in R if band[r]]):
                if bad:
                    return bad
    for r in R:                                    # back to the block layout: the zone's rows where there is a band, else every row
        bad = to_block(r, rowsel(0, zone) if band[r] else rowsel(0, ny))
        if bad:
            return bad
        if not (U[r] | ~(interior[r] | ghost[r])).all() or not (T[r] | ~(interior[r] | fringe[r])).all():
            return f"rank {r}: the call ends with a stale cell in the block layout"
    return None


@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ns", FOLDS)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_every_rank_plans_the_same_band_and_matching_lists(nx, ny, ns, shape, ext):
    dc = layout_of(nx, ny, ns, shape)
    Ls = plan_all(dc, ext=ext)
    top = ns == "tripoleT"
    for k in ("ext", "kpass", "ring_valid", "fold_zone", "fold_h", "list_row0", "band_ranks"):
        assert len({L[k] for L in Ls}) == 1, (k, [L[k] for L in Ls])
    L0 = Ls[0]
    zone, H, row0 = L0["fold_zone"], L0["fold_h"], L0["list_row0"]
    assert L0["ext"] == ext and zone + H == ny and H == ext + P + top and row0 == zone - (ext + P) and row0 >= 0
    # ... whatever tile height a rank's one-subcycle kernel has settled on (each rank times its own): it is no input of the plan
    for tyb in (3, 4, 8, 9):
        d, keep = evp.make_dims(dc, dc.nranks - 1)
        Lt = evp.march_layout(d, ext=ext, tyb=tyb)
        assert (Lt["fold_zone"], Lt["list_row0"], Lt["n_send"], Lt["n_recv"]) == (zone, row0, Ls[-1]["n_send"], Ls[-1]["n_recv"]), tyb
    own = owner_map(dc)
    for r, L in enumerate(Ls):
        oy, ox = np.nonzero(own == r)
        holds = oy.max() >= zone
        assert L["band_rows"] == (H if holds else 0), (r, L["band_rows"])
        assert L["nyo"] == min(oy.max() + 1, zone) - oy.min() and L["nyblk"] == oy.max() + 1 - oy.min()
        assert L["nxo"] == ox.max() + 1 - ox.min()
        if holds:
            assert oy.min() <= row0                       # the band's tile list lies inside the top row of ranks
    assert L0["band_ranks"] == shape[0] == sum(L["band_rows"] > 0 for L in Ls)
    corners = check_lists(dc, Ls)
    # a cut in x: the rank ring carries cells above the zone -- (ext + P) columns x (ext + P) rows on either side of every top rank
    assert corners == (2 * (ext + P) ** 2 * shape[0] if shape[0] > 1 else 0), corners
    for kpass, ndte in ((4, 24), (3, 25), (2, 24), (4, 33)):
        assert simulate(dc, Ls, ndte, kpass) is None, (kpass, ndte, simulate(dc, Ls, ndte, kpass))


@pytest.mark.parametrize("ns", FOLDS)
def test_several_blocks_per_rank_and_the_rim_search(ns):
    """2 x 2 ranks of 2 x 1 and of 2 x 2 blocks; not asked for a rim, every rank finds the same one (12 / 8 / 4 / 0) from the zone
    rectangles of all ranks."""
    for bpr in ((2, 1), (2, 2)):
        dc = layout_of(120, 80, ns, (2, 2), bpr)
        for ext in (4, None):
            Ls = plan_all(dc, ext=ext, tyb=5)
            for k in ("ext", "kpass", "fold_zone", "fold_h", "list_row0"):
                assert len({L[k] for L in Ls}) == 1, (k, [L[k] for L in Ls])
            L0 = Ls[0]
            if ext is None:
                assert L0["ext"] in (12, 8, 4, 0)
            check_lists(dc, Ls)
            assert simulate(dc, Ls, 24, L0["kpass"]) is None
    # the search narrows the rim where the widest is refused: four rows of ranks on 61 rows leave the top rank 8 rows of zone at most
    Ls = plan_all(layout_of(97, 61, ns, (1, 4)))
    assert {L["ext"] for L in Ls} == {0}


def test_the_simulation_sees_a_missing_corner():
    """The check checks: without the corner cells in the rank ring a top rank reads a stale cell for a cell it owns."""
    dc = layout_of(120, 80, "tripole", (2, 1))
    Ls = plan_all(dc, ext=0)
    assert simulate(dc, Ls, 24, 4) is None
    zone, nx = Ls[0]["fold_zone"], dc.nx_global
    cut = []
    for L in Ls:
        L = dict(L)
        gy, _ = cells_of(L, L["recv_pos1"], nx)
        keep = gy < zone
        assert (~keep).any()
        idx = np.nonzero(keep)[0]
        newcut = [int(np.searchsorted(idx, c)) for c in L["cut_recv"]]
        L["recv_pos1"], L["cut_recv"] = L["recv_pos1"][keep], np.array(newcut)
        cut.append(L)
    assert "stale" in (simulate(dc, cut, 24, 4) or "")
    # ... and with both halves of the trade before the ring, the zone rows reach the block layout's east fringe out of spent ring cells:
    # a velocity halo mends the ghost velocities, not the fringe stresses
    assert "stale" in (simulate(dc, Ls, 24, 4, ring_last=True) or "")


@pytest.mark.parametrize("ns", FOLDS)
def test_refusals_with_their_words(ns):
    # the top rank's share of the zone is thinner than rim + ring (then the band's list rows would reach into the rank below): every rank
    # says so -- 80 rows on 1 x 4 ranks with a rim of 8, 61 rows with a rim of 4
    for nx, ny, ext in ((120, 80, 8), (97, 61, 4)):
        dc = layout_of(nx, ny, ns, (1, 4))
        for r in range(4):
            d, keep = evp.make_dims(dc, r)
            with pytest.raises(evp.EvpHipError, match="share of the marched zone is thinner than its redundant rim \\+ ring: the fold band's list "
                                                      "rows do not lie inside the top row of ranks"):
                evp.march_layout(d, ext=ext)
    # eliminated land blocks, in the zone or in the band
    for dropped in ({(1, 1)}, {(2, 2)}):
        dc = drop(decomp.Decomp(120, 80, 30, 40, "cyclic", ns, 2, (2, 1)), dropped)
        for r in range(2):
            d, keep = evp.make_dims(dc, r)
            with pytest.raises(evp.EvpHipError, match="eliminated land blocks"):
                evp.march_layout(d, ext=4)
    # a grid too short for a zone under the band
    dc = layout_of(120, 14, ns, (2, 1))
    d, keep = evp.make_dims(dc, 0)
    with pytest.raises(evp.EvpHipError, match="too short"):
        evp.march_layout(d, ext=4)
    # ... and the one-rank entries keep their answer to several ranks
    dc = layout_of(120, 80, ns, (2, 1))
    d, keep = evp.make_dims(dc, 1)
    with pytest.raises(evp.EvpHipError, match="tripole grid on several ranks"):
        evp.march_plan(d, ext=4)
    with pytest.raises(evp.EvpHipError, match="tripole grid on several ranks"):
        evp.march_fold_plan(d, 4, 5)
