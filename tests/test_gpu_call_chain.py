"""GPU (-m gpu): a whole evp() call on the B grid -- cice_evp_hip_prep, the loop, cice_evp_hip_stress_halo, the download,
cice_evp_hip_deformations and cice_evp_hip_dyn_finish -- behind EVERY host of the loop: the streaming kernel, the on-chip resident
kernel (general, and where the lean variant is eligible), the marching kernel at four and three subcycles per pass, and on tripole /
tripoleT grids the marched zone beside its fold band.  The loop alone is pinned on each path elsewhere; here it is the hand-over that
is under test: the ping-pong buffer the loop ends on (S.cur after an odd count, after the band's flips), the final scatter of the
marching path (state, diagnostics, zone rows only beside a band), the ghost cells of the final velocities that deformations reads,
the marching host's ghost-cell check behind a preparation (upload_seq).  tests/evp_call_chain.py runs the chain and names the stage in
every message; every case asserts that its path ran (assert_path_ran).  Strict mode: bit for bit against the reference's fixtures and
the CPU oracle's chain; tests/test_call_chain_cpu.py shows without a GPU that these comparisons can see a stale ghost cell."""
import numpy as np
import pytest

import evp_call_chain as cc
from common import GoldenCase, assert_bitwise

pytestmark = pytest.mark.gpu

# Counts no fixture has, through the oracle's chain: the loop ends on the other ping-pong buffer.  Beside a fold band the block layout
# flips once per band subcycle: 7 = 4 + 3 is an odd number of them at four per pass (3 + 3 after a leading single one at three: even),
# 9 = 3 x 3 is odd at three per pass (1 + 4 + 4 at four: even) -- so each marching row ends on either buffer once.
ODD = (7, 9)


def fixture_rows():
    """Every fixture on every path; fold fixtures also with CICE_EVP_HIP_MARCH_EXT=0, which gives an 18-row grid a zone under its band --
    with the library's own rim some of the five still pass when the final scatter drops its diagnostics, with EXT=0 none does
    (profiles/r21_call_chain.txt).  The whole table costs 3 s, so no row waits behind common.wide()."""
    return [(n, p) for n in cc.chain_fixtures() for p in cc.LOOP_PATHS + (cc.FOLD_PATHS if cc.is_fold(GoldenCase(n).ns) else [])]


@pytest.mark.parametrize("name,path", fixture_rows())
def test_fixture_chain_on_every_path(name, path, monkeypatch):
    """Every call of the fixture and every subcycle count it has post-loop outputs for, on ONE core as consecutive evp() calls, then
    two odd counts through the oracle's chain."""
    cc.set_path(monkeypatch, path)
    c = GoldenCase(name)
    core = cc.open_core(c)
    try:
        for icall in range(1, c.ncalls + 1):
            for nsub in cc.post_counts(c):
                cc.run_chain(core, c, icall, nsub, path)
        for nsub in ODD:
            out = cc.run_chain(core, c, c.ncalls, nsub, path, reference="oracle")
            assert np.abs(out["uvel"]).max() > 0
    finally:
        core.finalize()


def synth_rows():
    rows = []
    for n, (ns, *_rest) in cc.SYNTH_CASES.items():
        paths = cc.LOOP_PATHS if ns == "closed" else ["marching k=4 ext=0", "marching k=3 ext=0", "marching k=4 ext=4", "marching k=3 ext=4"]
        rows += [(n, p) for p in paths]
    return rows


@pytest.mark.parametrize("name,path", synth_rows())
def test_synthetic_chain_vs_oracle(name, path, monkeypatch):
    """gx3- / tx3-sized grids, one block / 25 x 29 / 30 x 40 (padded) blocks, full cover / caps / independent holes: 9 subcycles
    (a leading single one, then passes) and 7 on one core; dyn_finish is handed a sentinel in both arrays."""
    cc.set_path(monkeypatch, path)
    case = cc.synth_case(name)
    core = case.open_core()
    try:
        for ndte in cc.SYNTH_NDTE:
            cc.run_synth_chain(core, case, ndte, path)
    finally:
        core.finalize()


@pytest.mark.parametrize("path", cc.LOOP_PATHS)
def test_two_calls_where_cells_lose_their_ice(path, monkeypatch):
    """The per-call entry as CICE would use it -- page-locked arrays, the stresses resident between the calls -- with cells that lose
    their ice between call 1 and call 2 (tests/evp_call_chain.py: TwoCalls; the fixture whose masks evolve loses two T-cells, this
    pair some thousands).  The caller's strintxU / strintyU / taubxU / taubyU enter call 2 with a sentinel off the new mask and come
    back as the oracle leaves them; the stresses fetched afterwards are the oracle's, zero off the new iceTmask; deformations and
    dyn_finish then run from the state the entry left on the device."""
    from cice_amd import evp
    cc.set_path(monkeypatch, path)
    t = cc.two_calls()
    b = t.base
    core = b.open_core()
    try:
        core.set_option(evp.OPT_STRESS_RESIDENT, 1)
        work = {k: np.zeros(core.shape) for k in evp.FIELDS}
        core.pin_host(*work.values())
        nonsig = [k for k in evp.OUTPUTS if k not in cc.SIG]
        for icall, (dyn, tm, um, want) in enumerate(((b.dyn, b.tm, b.um, t.out1), (t.dyn2, t.tm2, t.um2, t.want2["loop"])), 1):
            for k in evp.FIELDS:
                work[k][...] = np.nan if (icall == 2 and k in cc.SIG) else dyn[k]
            core.run_inplace(work, np.ascontiguousarray(tm, np.int32), np.ascontiguousarray(um, np.int32), t.ndte)
            # (16 blocks: the general resident kernel whatever the lean switch says)
            cc.assert_path_ran(core, path, t.ndte, False, False, f"call {icall} on {path}")
            assert_bitwise({k: work[k] for k in nonsig}, {k: want[k] for k in nonsig}, f"loop + masked download: call {icall} on {path}")
        sig = core.fetch_stresses()
        assert_bitwise(sig, {k: t.want2["loop"][k] for k in cc.SIG}, f"stresses fetched after call 2 on {path}")
        assert all(not sig[k][t.tm2 == 0].any() for k in cc.SIG), "stresses survive off the new iceTmask"
        assert_bitwise(core.deformations(), t.want2["deformations"], f"deformations: after call 2 on {path}")
        assert_bitwise(core.dyn_finish(*b.strocn), t.want2["dyn_finish"], f"dyn_finish: after call 2 on {path}")
    finally:
        core.finalize()


# ---- fused mode: deformations_kernel<false> / dyn_finish_kernel<false> ------------------------------------------------------------
def fused_call(monkeypatch, path):
    """The 100 x 116 holes case on a fused core behind `path`: (downloaded state, deformations, dyn_finish with the sentinel)."""
    cc.set_path(monkeypatch, path)
    case = cc.synth_case(cc.FUSED_CASE)
    core = case.open_core(strict=False)
    try:
        got = case.device_loop(core, cc.FUSED_NDTE)
        cc.assert_path_ran(core, path, cc.FUSED_NDTE, False, None, f"fused, {path}")
        return case, got, core.deformations(), core.dyn_finish(*case.strocn)
    finally:
        core.finalize()


def test_fused_post_loop_kernels_within_the_derived_bound(monkeypatch):
    """The fused build shares its bits with no reference: every ice cell of divu, shear, vort, rdg_conv, rdg_shear, strocnxU and
    strocnyU lies within n * 2^-53 * magnitude (tests/post_loop_ref.py: n counted from evp_cell.inc, not tuned) of the extended
    restatement evaluated on the device's OWN downloaded velocities; every cell off the ice is exactly 0 / the sentinel."""
    import post_loop_ref as R
    case, got, post, fin = fused_call(monkeypatch, "streaming")
    assert np.abs(got["uvel"]).max() > 1e-4
    worst = R.check(dict(post, **fin), got["uvel"], got["vvel"], case.static, case.post_geo, case.dyn, case.scal, case.blocks, case.tm,
                    case.um, cc.SENTINEL, "fused, streaming")
    print("\nfused post-loop kernels, worst |error| / bound:", {k: round(x, 3) for k, x in worst.items()})
    # ... and it IS another arithmetic than the strict build's: the oracle's bits are not reproduced on every cell
    want = case.oracle(cc.FUSED_NDTE)
    assert any(not np.array_equal(got[k], want["loop"][k]) for k in ("uvel", "vvel"))


def test_fused_call_behind_the_marching_kernel_equals_streaming(monkeypatch):
    """Contraction is per source expression, so the loop's bits are the same behind either host in fused mode
    (test_gpu_march.py); the post-loop calls that follow must then agree bit for bit as well."""
    _, a, pa, fa = fused_call(monkeypatch, "marching k=4")
    _, b, pb, fb = fused_call(monkeypatch, "streaming")
    assert_bitwise(a, b, "loop + download: fused, marching k=4 vs streaming")
    assert_bitwise(pa, pb, "deformations: fused, marching k=4 vs streaming")
    assert_bitwise(fa, fb, "dyn_finish: fused, marching k=4 vs streaming")
