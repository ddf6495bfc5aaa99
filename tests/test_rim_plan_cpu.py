"""CPU: the lane tables of the resident B-grid kernel's rim-wave schedule (cice_amd/csrc/rim_plan.cpp, read through the test
build's cice_evp_hip_rim_plan) against the rules of rim_plan.h restated in numpy.

A tile is 16 x 16 T-cell positions (trow*16 + tcol) and owns the U-cells of positions (0..14, 0..14) inside the block; T-cell
(r, c) reads the velocities of U-cells (r-1..r, c-1..c), U-cell (r, c) the stress partials of T-cells (r..r+1, c..c+1).  Chunk 0 is
the first 64 lanes.  "Held" is asked of every U-cell that does anything in the kernel -- it has ice, or it writes a record
because another tile polls it or it has a ghost image; an owned U-cell that has neither may be held by no lane (it sits at the
position of a chunk-0 padding lane, and no code touches it) -- the rule as rim_plan.h states it."""
import numpy as np
import pytest

from cice_amd import evp

W = 16
SIZES = [(15, 15), (16, 31), (31, 16), (37, 23), (100, 116)]


def _mask(kind, ni, nj):
    jj, ii = np.mgrid[0:nj + 2, 0:ni + 2]
    if kind == "all":
        t = u = np.ones((nj + 2, ni + 2), bool)
    elif kind == "diagonal":
        t = u = ii * (nj + 2) >= jj * (ni + 2)
    elif kind == "checker":
        t = u = (ii + jj) % 2 == 0
    elif kind == "one":
        t = u = (ii == min(ni, 9)) & (jj == min(nj, 7))
    else:
        rng = np.random.default_rng(int(kind))
        t = rng.random((nj + 2, ni + 2)) < 0.7
        u = rng.random((nj + 2, ni + 2)) < 0.7
    return (t.astype(np.uint8) | (u.astype(np.uint8) << 1)).astype(np.uint8)


def _geometry(ni, nj, cyclic_ew):
    """Per tile, from the block's shape alone: computed T positions, owned U positions, late T positions (read a velocity the
    tile does not produce and somebody else does), and per cell whether its record is polled or imaged."""
    ilo, ihi, jlo, jhi = 2, ni + 1, 2, nj + 1
    gx, gy = (ni + W - 2) // (W - 1), (nj + W - 2) // (W - 1)
    pub = np.zeros((nj + 3, ni + 3), bool)          # 1-based [j][i]
    if cyclic_ew:
        pub[jlo:jhi + 1, ilo] = pub[jlo:jhi + 1, ihi] = True
    tiles = []
    for by in range(gy):
        for bx in range(gx):
            i0, j0 = ilo + bx * (W - 1), jlo + by * (W - 1)
            computed, uown, late = np.zeros(256, bool), np.zeros(256, bool), np.zeros(256, bool)
            for pos in range(256):
                r, c = divmod(pos, W)
                i, j = i0 + c, j0 + r
                computed[pos] = i <= ihi + 1 and j <= jhi + 1
                uown[pos] = c < W - 1 and r < W - 1 and i <= ihi and j <= jhi
            for pos in np.nonzero(computed)[0]:
                r, c = divmod(int(pos), W)
                for dr in (0, 1):
                    for dc in (0, 1):
                        pr, pc, pi, pj = r - dr, c - dc, i0 + c - dc, j0 + r - dr
                        interior = ilo <= pi <= ihi and jlo <= pj <= jhi
                        if interior and 0 <= pr <= W - 2 and 0 <= pc <= W - 2:
                            continue
                        if interior:
                            pub[pj, pi] = late[pos] = True
                        elif cyclic_ew and jlo <= pj <= jhi:
                            pub[pj, pi + ni if pi < ilo else pi - ni] = late[pos] = True
            tiles.append((i0, j0, computed, uown, late))
    return gx, gy, tiles, pub


def _reads_t(u):      # T positions whose partials U position u reads
    r, c = divmod(u, W)
    return [(r + dr) * W + c + dc for dr in (0, 1) for dc in (0, 1)]


def _reads_u(t):      # U positions whose velocities T position t reads (may lie outside the tile's own 15 x 15)
    r, c = divmod(t, W)
    return [(r - dr) * W + c - dc for dr in (0, 1) for dc in (0, 1) if r - dr >= 0 and c - dc >= 0]


@pytest.mark.parametrize("kind", ["all", "diagonal", "checker", "one", "11", "12", "13"])
@pytest.mark.parametrize("ni,nj", SIZES)
def test_rim_plan_rules(ni, nj, kind):
    cyclic = (ni + nj) % 2 == 0          # both boundary types over the sizes
    mask = _mask(kind, ni, nj)
    P = evp.rim_plan(ni, nj, mask, cyclic_ew=cyclic)
    gx, gy, tiles, pub = _geometry(ni, nj, cyclic)
    assert (P["gx"], P["gy"]) == (gx, gy) and len(P["perm"]) == gx * gy
    for t, (i0, j0, computed, uown, late) in enumerate(tiles):
        perm, uperm = P["perm"][t].astype(int), P["uperm"][t].astype(int)
        cell = lambda pos: (j0 + pos // W - 1, i0 + pos % W - 1)          # 0-based index into mask
        ice = np.array([bool(computed[p] and mask[cell(p)] & 3) for p in range(256)])
        upub = np.array([bool(uown[p] and pub[j0 + p // W, i0 + p % W]) for p in range(256)])
        n = int(ice.sum())
        packed = (n + 63) // 64
        assert P["nact_packed"][t] == packed
        assert P["nact"][t] <= packed + 1, (t, P["nact"][t], packed)
        if kind == "all":
            assert P["ok"][t] and P["nact"][t] == packed, (t, P["nact"][t], packed)
        # none of these masks needs the fall-back: the rim cells and the edge U-cells of a 16 x 16 tile are at most 60 and 56, and a
        # tile with more than 192 + |L_T| ice cells has ice on so much of its rim that the fill-up stays within L_U's 64 lanes
        assert P["ok"][t], (t, P["n_lt"][t], P["n_lu"][t])
        # every T-cell position, so every ice T-cell, is held by exactly one lane; ice first
        assert sorted(perm) == list(range(256))
        assert not ice[perm[64 * P["nact"][t]:]].any()
        lt = {p for p in perm[:64] if ice[p]}
        lu = {u for u in uperm[:64] if u != 255}
        assert len(lt) == P["n_lt"][t] <= 64 and len(lu) == P["n_lu"][t] <= 64
        assert {p for p in range(256) if ice[p] and late[p]} <= lt
        # U-cells: no cell twice, owned cells only, everything that takes part exactly once; outside chunk 0 a lane's U-cell is
        # the one at its T-cell's position
        held = [u for u in uperm if u != 255]
        assert len(held) == len(set(held)) and all(uown[u] for u in held)
        for u in np.nonzero(uown)[0]:
            if u not in held:
                assert not ice[u] and not upub[u], (t, u)
        assert all(uperm[l] in (255, perm[l]) for l in range(64, 256))
        assert {u for u in range(256) if upub[u]} <= lu
        # no U-cell outside L_U reads a T-cell of L_T (the other positions chunk 0 holds have no ice: their partials are never
        # written and stay zero)
        for u in held:
            if u not in lu:
                assert not (set(_reads_t(u)) & lt), (t, u)
        # no T-cell of L_T reads the velocity of a U-cell of this tile outside L_U
        for p in lt:
            for u in _reads_u(p):
                if u // W <= W - 2 and u % W <= W - 2 and uown[u]:
                    assert u in lu, (t, p, u)
