"""CPU: what the host of the marching path decides from the dims and a few asked-for integers alone (cice_amd/csrc/march_plan.cpp:
build_march_layout, read through the test build's cice_evp_hip_march_layout) against the rules restated in numpy.  The same
function builds the layout evp_host_march.cpp uploads and allocates by, so a changed decision shows here, without a GPU.

The rules (P = 4 cells of overlap, strips own at most 56 columns):
  rim     the widest of 12 / 8 / 4 / 0 cells the plan accepts (no rank closer to a closed boundary than rim + P) that costs no rank a
          strip more than a rim of 4 does and at most 2 % more rows; 4 and 0 are taken as soon as the plan accepts them
  K       subcycles per pass by the SHORTEST segment of any rank (1024 waves over its strips, at least 6 rows): 4 from 12 rows, 3 from
          8, 2 below -- on several ranks the rim counts on both sides, whether the rank has a neighbour there or not
  sizes   ldx = strips * own + 64 + 2P rounded up to 8, rows = nyr + 2P + 3, nblk = rows * strips, 14 * 512 * nblk < 2^32;
          segments of max(6, ceil(nyr / (1024 // strips))) rows
  items   per strip, runs of rows that hold a sent cell, at most max(6, seglen // 3) long (band), and of the others, at most seglen"""
import types

import numpy as np
import pytest

from cice_amd import decomp, evp
from test_multirank_cpu import MARCH_CASES

P, OWN, NF, NODUP = 4, 56, 14, 0xFFFFFFFF


def layout(dc, rank=0, **ask):
    d, keep = evp.make_dims(dc, rank)
    return evp.march_layout(d, **ask)


def rects(dc):
    """every rank's own cells as (gx0, gy0, nxr, nyr), 0-based"""
    out = []
    for r in range(dc.nranks):
        b = dc.local_blocks(r)
        x0, y0 = min(q.gi0 for q in b) - 1, min(q.gj0 for q in b) - 1
        out.append((x0, y0, max(q.gi0 + q.gnx for q in b) - 1 - x0, max(q.gj0 + q.gny for q in b) - 1 - y0))
    return np.array(out)


def rim_rule(dc):
    R, cyc = rects(dc), dc.ew == "cyclic"
    x0, y0, nxr, nyr = R.T
    west, east, south, north = x0, dc.nx_global - (x0 + nxr), y0, dc.ny_global - (y0 + nyr)      # cells to the global boundary
    span = cyc & (nxr == dc.nx_global)                                                            # wraps inside: no rim in x
    sides_x = np.where(span, 0, ((west > 0) | cyc).astype(int) + ((east > 0) | cyc))
    sides_y = (south > 0).astype(int) + (north > 0)
    for e in (12, 8, 4, 0):
        thin = [(dd > 0) & (dd < e + P) for dd in (west, east, south, north)]
        if ((thin[0] | thin[1]) & (not cyc)).any() or (thin[2] | thin[3]).any():
            continue
        if e <= 4:
            return e
        strips = lambda w: -(-(nxr + w * sides_x) // OWN)
        rows = lambda w: nyr + w * sides_y
        if (strips(e) <= strips(4)).all() and (rows(e) * 100 <= rows(4) * 102).all():
            return e
    return None


def k_rule(dc, ext):
    x0, y0, nxr, nyr = rects(dc).T
    grow = 2 * ext if dc.nranks > 1 else 0
    nseg = np.maximum(1, 1024 // -(-(nxr + grow) // OWN))
    sl = np.maximum(6, -(-(nyr + grow) // nseg)).min()
    return 4 if sl >= 12 else 3 if sl >= 8 else 2


def check_sizes(L, seglen=0):
    assert L["ring_valid"] == L["ext"] + P
    assert L["nstrips"] == -(-L["nxr"] // L["own"]) and L["own"] <= OWN
    assert L["ldx"] == -(-(L["nstrips"] * L["own"] + 64 + 2 * P) // 8) * 8
    assert L["rows"] == L["nyr"] + 2 * P + 3 and L["nblk"] == L["rows"] * L["nstrips"]
    assert L["nblk"] * NF * 512 < 2 ** 32
    want = seglen or max(6, -(-L["nyr"] // max(1, 1024 // L["nstrips"])))
    assert L["seglen"] == min(want, L["nyr"])
    assert L["nseg"] == -(-L["nyr"] // L["seglen"]) and L["nitems"] == L["nseg"] * L["nstrips"]
    # a duplicate is another lane that holds the same column (through the wrap of the strips, where they wrap)
    s, l = np.nonzero(L["dup"] != NODUP)
    off = L["dup"][s, l].astype(np.int64)
    assert (off % 8 == 0).all()
    s2, l2 = off // 8 // (NF * 64), off // 8 % (NF * 64)
    assert (l2 < 64).all() and (s2 < L["nstrips"]).all() and ((s2 != s) | (l2 != l)).all()
    shift = (s2 * L["own"] + l2) - (s * L["own"] + l)
    assert np.isin(shift, (0, L["nxr"], -L["nxr"]) if L["wrapx"] else (0,)).all()


# ---- rim and K ------------------------------------------------------------------------------------------------------------
BIG = {}


def big(shape):
    """3600 x 2400, cyclic / closed, as one rank or as px x py cyclic pieces (rank 0's layout; its lists are built once)"""
    if shape not in BIG:
        px, py = shape
        dc = decomp.Decomp(3600, 2400, 3600 // px, 2400 // py, "cyclic", "closed", px * py, shape)
        BIG[shape] = (dc, layout(dc, 0))
    return BIG[shape]


def test_rim_3600x2400_one_rank_known_answer():
    """65 strips x 15 segments of 160 rows, four subcycles per pass; no neighbour, so the widest rim costs nothing"""
    dc, L = big((1, 1))
    assert (L["ext"], L["npeers"], L["n_send"], L["nband"], L["nrest"]) == (12, 0, 0, 0, 0)
    assert (L["nstrips"], L["nseg"], L["seglen"], L["kpass"]) == (65, 15, 160, 4)
    assert (L["nxr"], L["nyr"], L["ext_w"], L["ext_s"], L["wrapx"]) == (3600, 2400, 0, 0, 1)
    assert rim_rule(dc) == 12 and k_rule(dc, 12) == 4
    check_sizes(L)


@pytest.mark.parametrize("shape", [(8, 1), (4, 2)])
def test_rim_3600x2400_pieces_keep_the_widest_rim(shape):
    """8 x 1: 450 + 2 x 12 = 474 columns still fit the 9 strips that 458 need"""
    dc, L = big(shape)
    assert L["ext"] == 12 == rim_rule(dc) and L["kpass"] == 4 == k_rule(dc, 12)
    if shape == (8, 1):
        assert (L["nxr"], L["nstrips"], -(-458 // OWN)) == (474, 9, 9)
    check_sizes(L)


THIN = [
    # nx, ny, proc shape, rim: what the wider rims would cost
    (192, 60, (2, 1), 8),       # 96 columns + 2 x 12 = 120 need 3 strips, + 2 x 8 = 112 the 2 that 104 need
    (200, 60, (2, 1), 4),       # 100 columns: + 2 x 8 = 116 need 3 strips against 2 for 108
    (112, 600, (1, 2), 8),      # 300 rows and one neighbour: 312 > 1.02 x 304, 308 is not
    (112, 300, (1, 2), 4),      # 150 rows: 158 > 1.02 x 154
    (224, 800, (2, 4), 4),      # 200 rows, the inner ranks with two neighbours: 216 > 1.02 x 208
]


@pytest.mark.parametrize("nx,ny,shape,rim", THIN)
def test_rim_narrower_where_the_widest_costs_a_strip_or_rows(nx, ny, shape, rim):
    dc = decomp.Decomp(nx, ny, nx // shape[0], ny // shape[1], "cyclic", "closed", shape[0] * shape[1], shape)
    assert rim_rule(dc) == rim
    for rank in range(dc.nranks):
        L = layout(dc, rank)
        assert L["ext"] == rim and L["kpass"] == k_rule(dc, rim), (rank, L["ext"], L["kpass"])
        check_sizes(L)


def test_rim_of_a_rank_too_thin_next_to_a_closed_boundary():
    """the layouts of test_march_plan_refuses_a_rank_too_thin_next_to_a_closed_boundary: an asked-for rim is refused with the
    plan's words; the search falls back to no rim where the ring alone fits, and reports the widest rim's error where nothing does"""
    dc = decomp.Decomp(40, 24, 36, 24, "closed", "closed", 2, (2, 1))           # the east rank is 4 columns wide
    for rank in (0, 1):
        with pytest.raises(evp.EvpHipError, match="march layout: a rank lies closer to a closed boundary than its redundant rim"):
            layout(dc, rank, ext=4)
        assert rim_rule(dc) == 0 and layout(dc, rank)["ext"] == 0
        assert layout(dc, rank, ext=0)["ring_valid"] == P
    dc = decomp.Decomp(39, 24, 36, 24, "closed", "closed", 2, (2, 1))           # 3 columns: thinner than the ring itself
    assert rim_rule(dc) is None
    for rank in (0, 1):
        with pytest.raises(evp.EvpHipError, match="closer to a closed boundary|too small"):
            layout(dc, rank)


@pytest.mark.parametrize("nx,ny,k", [(3600, 2400, 4), (560, 1200, 4), (560, 1000, 3), (560, 800, 3), (560, 700, 2), (560, 500, 2)])
def test_k_rule_one_rank(nx, ny, k):
    """560 columns = 10 strips, 102 segments: 12, 10, 8, 7 and 6 (the least) rows per segment"""
    dc, L = big((1, 1)) if nx == 3600 else (decomp.Decomp(nx, ny, nx, ny, "cyclic", "closed"), None)
    L = L or layout(dc)
    assert L["kpass"] == k == k_rule(dc, L["ext"])
    check_sizes(L)


def test_k_rule_looks_at_the_shortest_segment_of_any_rank():
    """rows 0 .. 1799 and 1800 .. 2399 of 560 columns, rim 12: 11 strips with the rim on both sides, 93 segments -- 20 rows on rank
    0, 7 on rank 1, so two subcycles per pass on both"""
    dc = decomp.Decomp(560, 2400, 560, 600, "cyclic", "closed", 2, (1, 2))
    for b in dc.blocks:
        b.owner, b.local = (0, b.jblock - 1) if b.jblock < 4 else (1, 0)
    assert [len(dc.local_blocks(r)) for r in (0, 1)] == [3, 1]
    ext = rim_rule(dc)
    for rank in (0, 1):
        L = layout(dc, rank)
        assert (L["ext"], L["kpass"]) == (ext, k_rule(dc, ext)) == (12, 2), (rank, L["ext"], L["kpass"])
        check_sizes(L)


def test_tripole_3600x2400_one_rank_known_answer():
    """DESIGN.md, section 4 (marched zone + fold band): H = 18, ext = 12, 65 strips x 15 segments -- with tiles 8 rows high, whose 7
    U-rows put the first row of the band's list on row 2366"""
    dc = decomp.Decomp(3600, 2400, 3600, 2400, "cyclic", "tripole")
    L = layout(dc, tyb=8)
    assert (L["fold_h"], L["ext"], L["fold_zone"] + L["fold_h"]) == (18, 12, 2400)
    assert (L["nyo"], L["nyr"], L["nyblk"], L["ext_s"]) == (2382, 2382 + 12, 2400, 0)     # the zone, its rim above; the blocks go on
    assert (L["nstrips"], L["nseg"], L["kpass"], L["npeers"]) == (65, 15, 4, 0)
    check_sizes(L)


def test_what_is_asked_for_is_clamped():
    dc = decomp.Decomp(192, 60, 96, 60, "cyclic", "closed", 2, (2, 1))
    assert layout(dc, ext=6)["ext"] == 6 and layout(dc, ext=5)["ext"] == 4 and layout(dc, ext=-3)["ext"] == 0
    assert layout(dc, kpass=7)["kpass"] == 4 and layout(dc, kpass=1)["kpass"] == 2 and layout(dc, kpass=3)["kpass"] == 3
    check_sizes(layout(dc, seglen=10), seglen=10)
    check_sizes(layout(dc, seglen=1000), seglen=1000)
    assert layout(dc, own_max=20)["own"] <= 20


# ---- the ring's lists and the items of an overlapped exchange pass ----------------------------------------------------------
@pytest.mark.parametrize("case", MARCH_CASES)
@pytest.mark.parametrize("bandseg", [0, 3])
def test_band_and_rest_items_cover_the_rectangle_once(case, bandseg):
    nx, ny, bx, by, ew, nranks, shape, own_max, wrap_inside, ext = case
    dc = decomp.Decomp(nx, ny, bx, by, ew, "closed", nranks, shape)
    for rank in range(nranks):
        d, keep = evp.make_dims(dc, rank)
        L = evp.march_layout(d, own_max, wrap_inside, ext, bandseg=bandseg)
        check_sizes(L)
        ns, nyr = L["nstrips"], L["nyr"]
        cover = np.zeros((2, ns, nyr), dtype=int)
        for which, items, most in ((0, L["band_items"], bandseg or max(6, L["seglen"] // 3)), (1, L["rest_items"], L["seglen"])):
            assert (which or len(items) > 0) and (items[:, 3] == 0).all()
            assert (items[:, 2] > items[:, 1]).all() and (items[:, 2] - items[:, 1] <= most).all(), (rank, which, most)
            for st, y0, y1, _ in items:
                cover[which, st, y0:y1] += 1
        assert (cover[0] * cover[1] == 0).all(), "band and rest items share a (strip, row)"
        assert (cover.sum(axis=0) == 1).all(), "a (strip, row) of the held rectangle is covered twice or not at all"
        # every sent cell lies in a band item, and only rows that hold one do
        blk = L["send_pos"] >> 6
        strip, y = blk % ns, blk // ns - P
        assert ((y >= 0) & (y < nyr)).all() and (cover[0, strip, y] == 1).all()
        sent = np.zeros((ns, nyr), dtype=int)
        sent[strip, y] = 1
        assert (sent == cover[0]).all()
        # the flat lists are the plan's, peer after peer; the byte mask is row-major with P halo columns
        pl = evp.march_plan(d, own_max, wrap_inside, ext)
        for k in ("send_pos", "recv_pos1", "recv_pos2"):
            assert np.array_equal(L[k], pl[k]), k
        assert np.array_equal(L["cut_send"], np.concatenate(([0], np.cumsum(pl["peer_nsend"]))))
        assert np.array_equal(L["cut_recv"], np.concatenate(([0], np.cumsum(pl["peer_nrecv"]))))
        for pos, midx in ((L["send_pos"], L["send_midx"]), (L["recv_pos1"], L["recv_midx"])):
            b, lane = pos >> 6, pos & 63
            assert np.array_equal(midx, (b // ns) * L["ldx"] + (b % ns) * L["own"] + lane)      # column = strip * own + lane - P


# ---- the block grid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,shape", [(1, (1, 1)), (2, (2, 1)), (2, (1, 2))])
def test_block_tables_invert_each_other(nranks, shape):
    """blocks of 30 x 20 on 200 x 70: the last block column is 20 wide, the last block row 10 high"""
    dc = decomp.Decomp(200, 70, 30, 20, "cyclic", "closed", nranks, shape)
    R = rects(dc)
    for rank in range(nranks):
        L = layout(dc, rank)
        check_sizes(L)
        blocks = dc.local_blocks(rank)
        assert (L["bsx"], L["bsy"]) == (30, 20) and L["nbx"] * L["nby"] == len(blocks) == L["norg"]
        assert (L["nxo"], L["nyo"], L["nyblk"]) == (R[rank][2], R[rank][3], R[rank][3])
        assert (L["gx0"], L["gy0"]) == (R[rank][0] - L["ext_w"], R[rank][1] - L["ext_s"])
        assert sorted(L["blkid"].ravel()) == list(range(len(blocks)))
        for bj in range(L["nby"]):
            for bi in range(L["nbx"]):
                b = L["blkid"][bj, bi]
                assert tuple(L["org"][b]) == (bi * 30 + L["ext_w"], bj * 20 + L["ext_s"])
                assert (blocks[b].gi0 - 1 - R[rank][0], blocks[b].gj0 - 1 - R[rank][1]) == (bi * 30, bj * 20)
        assert len({(b.gnx, b.gny) for b in blocks}) > 1                  # a smaller last column and / or row on this rank


def edited(dc, local):
    """`dc` with another list of local blocks on rank 0 (the global block table stays as it is)"""
    return types.SimpleNamespace(nx_block=dc.nx_block, ny_block=dc.ny_block, nx_global=dc.nx_global, ny_global=dc.ny_global, ew=dc.ew,
                                 ns=dc.ns, nranks=dc.nranks, blocks=dc.blocks, local_blocks=lambda rank: local)


def test_refusals_of_the_block_grid():
    dc = decomp.Decomp(90, 60, 30, 20, "cyclic", "closed")
    nine = dc.local_blocks(0)
    with pytest.raises(evp.EvpHipError, match="march layout: blocks do not tile a rectangle"):
        layout(edited(dc, nine[:4] + nine[5:]))                         # the centre block is missing
    narrow = [decomp.Block(b.gid, b.iblock, b.jblock, b.gi0, b.gj0, b.gnx - 10 * (k == 4), b.gny, 0, k) for k, b in enumerate(nine)]
    with pytest.raises(evp.EvpHipError, match="march layout: irregular block sizes"):
        layout(edited(dc, narrow))                                      # the centre block is 20 columns wide in a slot of 30
    dc = decomp.Decomp(90, 60, 30, 20, "cyclic", "closed")
    assert layout(dc)["nbx"] == 3                                        # (the same domain, untouched, is accepted)


def test_refuses_a_state_buffer_beyond_32_bit_byte_offsets():
    """14 fields x 512 bytes per (row, strip): 2^32 bytes are 599186.3 of them.  1000 strips: 599 rows fit, 600 do not -- held as
    dims only"""
    L = layout(decomp.Decomp(56000, 588, 56000, 588, "closed", "closed"))
    assert (L["nstrips"], L["rows"], L["nblk"]) == (1000, 599, 599000)
    with pytest.raises(evp.EvpHipError, match="march layout: state buffer beyond 32-bit byte offsets"):
        layout(decomp.Decomp(56000, 589, 56000, 589, "closed", "closed"))
