"""CPU: how the marching path shares a tripole grid on one rank between the marched zone (rows 0 .. zone-1, several subcycles
per pass in the strip-major rectangle) and the fold band (the top H rows, one subcycle per launch in the block layout), through
the host-only entry cice_evp_hip_march_fold_plan (cice_amd/csrc/march_plan.cpp: build_march_fold).

The rule both sides live by is restated here: a subcycle computes row r from rows r-1, r, r+1 of the state before it
(stress of T-row r reads the velocities of rows r-1 and r, stepu of U-row r the stresses of T-rows r and r+1), so a side that
computes a range of rows from a state that is current on a range loses one row per subcycle at every end that is not a
boundary.  The ring exchange copies rows that are current on the side that owns them to the side that only reads them."""
import numpy as np
import pytest

from cice_amd import decomp, evp
from common import GoldenCase

P = 4                      # EVP_MARCH_PAD
EXTS = (0, 4, 8, 12)


def dims_of(nx, ny, bsx, bsy, ns="tripole", nranks=1):
    dc = decomp.Decomp(nx, ny, bsx, bsy, "cyclic", ns, nranks)
    d, keep = evp.make_dims(dc, 0)
    blocks = [(b.gj0 - 1, b.gny) for b in dc.local_blocks(0)]
    return d, keep, blocks, ny


def fixture_dims(name):
    c = GoldenCase(name)
    d, keep = c.hip_dims()
    blocks = [(int(c.blk[b, 7]) - 1, int(c.blk[b, 3]) - int(c.blk[b, 2]) + 1) for b in range(c.nblocks)]
    return d, keep, blocks, c.ny_global


def simulate(plan, ny, kpass, nsub, to_block=None, to_rect=None):
    """Both sides over nsub subcycles with the host's schedule: the very steps march_run iterates over (march_plan.cpp:
    march_schedule -- passes of kpass; the ring is exchanged when fewer valid rows are left than the next pass advances).  Returns
    None, or what went wrong."""
    zone, ext = plan["zone"], plan["ext"]
    to_block = to_block or plan["to_block"]
    to_rect = to_rect or plan["to_rect"]
    held = plan["rect_rows"]                       # rows the rectangle advances; it reads P more above them
    zvalid = set(range(0, held + P))               # the gather at the start of a call fills all of it
    bvalid = set(range(0, ny))                     # the block layout is complete then
    for k, _, fexch, _ in evp.march_schedule(nsub, kpass, ext + P, False, True):
        if k == 1:                                 # (the host runs a single left-over subcycle first, over the whole domain)
            continue
        # The zone's pass advances k subcycles at once: the levels in between live in the kernel (it evaluates them on the ring
        # rows too, as far as they are valid) and only rows below `held` are stored -- a stored row is current when the k rows
        # on either side of it were.  South of row 0 lies the closed boundary.
        zvalid = {r for r in range(0, held) if all(q in zvalid for q in range(max(r - k, 0), r + k + 1))}
        if not set(range(0, zone)) <= zvalid:
            return f"the zone lost one of its own rows (valid up to {max(zvalid)})"
        for _ in range(k):
            # the band, one subcycle at a time; north of row ny-1 lies the ghost row, which its halo step keeps current
            bvalid = {r for r in range(plan["list_row0"], ny)
                      if r - 1 in bvalid and r in bvalid and (r == ny - 1 or r + 1 in bvalid)}
            if not set(range(zone, ny)) <= bvalid:
                return f"the band lost one of its own rows (valid from {min(bvalid)})"
        if fexch:
            src_b, src_r = set(range(*to_block)), set(range(*to_rect))
            if not src_b <= zvalid:
                return "the exchange copied a stale row of the rectangle into the block layout"
            if not src_r <= bvalid:
                return "the exchange copied a stale row of the block layout into the rectangle"
            bvalid |= src_b
            zvalid |= src_r
    return None


def countdown(ndte, kpass, ring_valid, has_peers, fold):
    """The schedule restated: a single left-over subcycle first, passes of kpass, the remaining 2 .. kpass - 1; every pass costs its
    size in valid cells beyond the rank's own, and what is left of the P-cell ring after a pass is a state older; the ring travels
    when the next pass needs more than there is (and, between ranks, after the last pass)."""
    steps = [(1, False, False, False)] if ndte % kpass == 1 else []
    sizes = np.array([kpass] * (ndte // kpass) + ([ndte % kpass] if ndte % kpass > 1 else []), dtype=int)
    valid = ring_valid
    for i, size in enumerate(sizes):
        last = i == len(sizes) - 1
        valid = min(valid - size, ring_valid - P)
        spent = not last and valid < sizes[i + 1]
        steps.append((int(size), has_peers and (last or spent), fold and spent, last))
        if steps[-1][1] or steps[-1][2]:
            valid = ring_valid
    return steps


@pytest.mark.parametrize("kpass", (2, 3, 4))
def test_schedule_sizes_and_countdown(kpass):
    for ndte in range(1, 41):
        for ext in EXTS:
            for has_peers in (False, True):
                for fold in (False, True):
                    st = evp.march_schedule(ndte, kpass, ext + P, has_peers, fold)
                    what = (ndte, kpass, ext, has_peers, fold, st)
                    assert sum(s[0] for s in st) == ndte, what
                    assert all(s[0] >= 2 for s in st[1:]) and all(1 <= s[0] <= kpass for s in st), what
                    assert st == countdown(ndte, kpass, ext + P, has_peers, fold), what
                    if st[0][0] == 1:
                        assert st[0][1:] == (False, False, False), what
                    passes = [s for s in st if s[0] > 1]
                    assert [s[3] for s in passes] == [False] * (len(passes) - 1) + [True] * bool(passes), what
                    # no pass runs on fewer valid cells than it advances: between two exchanges at most ring_valid subcycles
                    if has_peers or fold:
                        run = 0
                        for size, exch, fexch, last in passes:
                            run += size
                            assert run <= ext + P, what
                            if exch or fexch:
                                run = 0


def check_plan(d, blocks, ny, ext, tyb, tfold=False):
    """tfold (tripoleT): the top physical row holds images whose cell areas are not dxT * dyT in CICE's arrays -- the zone's ring
    stays below it, so the band is at least one row taller."""
    if ny < 2 * (ext + P) + tfold:
        with pytest.raises(evp.EvpHipError, match="too short"):
            evp.march_fold_plan(d, ext, tyb)
        return None
    pl = evp.march_fold_plan(d, ext, tyb)
    zone, h = pl["zone"], pl["band_rows"]
    what = (ny, ext, tyb, pl)
    # every physical row has one owner
    owner = np.zeros(ny, dtype=int)
    owner[:zone] += 1
    owner[ny - h:] += 1
    assert (owner == 1).all() and zone >= 1, what
    assert h >= ext + P + tfold, what
    assert pl["rect_rows"] == zone + ext and pl["rect_rows"] + P <= ny - tfold, what   # the ring lies on physical rows
    assert pl["tile_rows_height"] == tyb - 1
    # the band's list reaches ext + P rows below its own: every row from there up is in a tile of the block that holds it,
    # and the last tile row of a block also owns the T-row jhi + 1
    assert pl["list_row0"] <= zone - (ext + P) and pl["list_row0"] >= 0, what
    t = tyb - 1
    for (gj0, gny), (by0, by1) in zip(blocks, pl["tile_rows"]):
        rows = set()
        for by in range(by0, by1):
            rows |= set(range(gj0 + by * t, gj0 + min((by + 1) * t, gny)))
        need = set(r for r in range(gj0, gj0 + gny) if r >= pl["list_row0"])
        assert need <= rows, (what, gj0, gny, by0, by1)
        if need:
            assert by1 * t >= gny and by0 * t + gj0 <= max(pl["list_row0"], gj0), (what, gj0, gny, by0, by1)
        else:
            assert by0 == by1, (what, gj0, gny, by0, by1)
    assert pl["to_block"] == (zone - (ext + P), zone) and pl["to_rect"] == (zone, zone + ext + P), what
    # no stale row is ever read for an owned cell, whatever the pass size and the count
    for kpass in (2, 3, 4):
        for nsub in (14, 33, 60):
            assert simulate(pl, ny, kpass, nsub) is None, (what, kpass, nsub, simulate(pl, ny, kpass, nsub))
    # ... and the windows are no larger than that needs: one row less on either side and a side loses a row it owns
    # (passes of four with ext a multiple of four: exactly ext + P subcycles between two exchanges)
    lo, hi = pl["to_block"]
    assert simulate(pl, ny, 4, 60, to_block=(lo + 1, hi)) is not None or pl["list_row0"] < lo, what
    lo, hi = pl["to_rect"]
    assert simulate(pl, ny, 4, 60, to_rect=(lo, hi - 1)) is not None, what
    return pl


@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("nx,ny,bs", [(360, 240, (360, 240)), (360, 240, (90, 60)), (360, 240, (100, 37)),
                                      (3600, 2400, (3600, 2400)), (3600, 2400, (900, 600))])
def test_fold_plan_tx1_and_full_size(nx, ny, bs, ext):
    d, keep, blocks, ny = dims_of(nx, ny, *bs)
    for tyb in (5, 9, 2):
        pl = check_plan(d, blocks, ny, ext, tyb)
        assert pl is not None
        # H is ext + P rounded up to a tile row of the block that holds the first row of the list: never a whole tile row more
        assert pl["band_rows"] < ext + P + (tyb - 1), pl


@pytest.mark.parametrize("ext", EXTS)
@pytest.mark.parametrize("name", ["trip_cyc_2x2_full", "trip_cyc_1blk_patchy", "trip_cyc_4x3_caps", "tript_cyc_2x2_full",
                                  "tript_cyc_1blk_patchy"])
def test_fold_plan_fixture_sizes(name, ext):
    """28 x 20, 24 x 18 and 32 x 24: each has a zone at ext = 0 (the plan accepts NY >= 16 there)."""
    d, keep, blocks, ny = fixture_dims(name)
    for tyb in (5, 3, 8):
        pl = check_plan(d, blocks, ny, ext, tyb, tfold=name.startswith("tript_"))
        if ext == 0:
            assert pl is not None and pl["zone"] >= P


@pytest.mark.parametrize("seed", range(40))
def test_fold_plan_random_sizes_and_cuts(seed):
    rng = np.random.default_rng(seed)
    nx, ny = int(rng.integers(16, 400)), int(rng.integers(16, 300))
    nbx, nby = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    bsx, bsy = -(-nx // nbx), -(-ny // nby)
    ns = "tripole" if seed % 2 else "tripoleT"
    d, keep, blocks, ny = dims_of(nx, ny, bsx, bsy, ns=ns)
    tyb = int(rng.integers(2, 10))
    accepted = 0
    for ext in EXTS:
        accepted += check_plan(d, blocks, ny, ext, tyb, tfold=(ns == "tripoleT")) is not None
    assert accepted >= 1               # NY >= 16: ext = 0 always fits


def test_fold_plan_refuses_several_ranks_closed_and_cyclic_grids():
    dc = decomp.per_rank_blocks(360, 240, 2, "cyclic", "tripole", proc_shape=(2, 1))
    d, keep = evp.make_dims(dc, 0)
    with pytest.raises(evp.EvpHipError, match="tripole grid on several ranks"):
        evp.march_fold_plan(d, 4, 5)
    with pytest.raises(evp.EvpHipError, match="tripole grid on several ranks"):
        evp.march_plan(d, ext=4)                      # the marching path stays off on every rank, and says why
    for ns in ("closed", "cyclic"):
        d, keep, blocks, ny = dims_of(120, 80, 60, 40, ns=ns)
        with pytest.raises(evp.EvpHipError, match="no tripole fold"):
            evp.march_fold_plan(d, 4, 5)
    d, keep, blocks, ny = dims_of(120, 80, 60, 40, ns="cyclic")
    with pytest.raises(evp.EvpHipError, match="not closed"):
        evp.march_plan(d, ext=4)
    d, keep, blocks, ny = dims_of(120, 80, 60, 40, ns="tripole")
    with pytest.raises(evp.EvpHipError, match="not closed"):
        evp.march_plan(d, ext=4)                      # (the plan of a closed rectangle: a tripole grid needs its band)
