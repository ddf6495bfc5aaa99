"""The halo plan (cice_amd/csrc/halo_plan.cpp: build_halo_plan), byte for byte: a SHA-256 per case over what the test build's
cice_evp_hip_plan_dump hands out -- every member of HaloPlan in declaration order, peers and the C grid's fold lists included -- for
every rank of the case in rank order; where cice_evp_hip_plan_build refuses a rank's description, the text of cice_evp_hip_last_error
stands in for the dump.

The expected digests were recorded from the planner of the commit BEFORE build_halo_plan was rewritten as a sequence of steps over one
ghost-cell walk, one boundary rule and one peer recorder (the dump entry put on that commit's halo_plan.cpp, untouched), with this
file's own digest function; they pin that the rewrite moved no list entry.  tests/test_multirank_cpu.py, test_cgrid_fold_split_cpu.py,
test_capi_cpu.py and the plan cases of test_oracle_golden.py stay the independent statement of what the lists mean; this file only
says "as before".  A deliberate change of the plan (a new layout, a new list) re-records the literals it changes, and says so.
"""
import ctypes as C
import hashlib

import pytest

from cice_amd import decomp, evp

import test_cgrid_fold_split_cpu as fold_cases
import test_multirank_cpu as multirank_cases

EW = ("closed", "open", "cyclic")
NS = ("closed", "open", "cyclic", "tripole", "tripoleT")
SPLIT_SHAPES = [(2, 1), (3, 1), (4, 1), (2, 2), (4, 2)]      # of test_fold_row_split_over_ranks_lists_of_the_on_chip_kernel, 48 x 20
HALO_CASES = [                                               # of test_cgrid_fold_split_cpu.py, as recorded
    (72, 40, 36, 40, "tripole", 2, (2, 1), None),
    (72, 40, 18, 40, "tripole", 4, (4, 1), None),
    (72, 40, 25, 40, "tripole", 3, (3, 1), None),
    (72, 40, 12, 10, "tripole", 4, (2, 2), None),
    (72, 40, 72, 13, "tripole", 2, None, ("top", 1)),
    (72, 40, 18, 10, "tripole", 2, (2, 1), ("drop", 2)),
    (72, 40, 36, 40, "tripoleT", 2, (2, 1), None),
    (72, 40, 18, 40, "tripoleT", 4, (4, 1), None),
    (72, 40, 25, 40, "tripoleT", 3, (3, 1), None),
    (72, 40, 12, 10, "tripoleT", 4, (2, 2), None),
    (72, 40, 72, 19, "tripoleT", 2, None, ("top", 1)),
    (72, 40, 18, 10, "tripoleT", 2, (2, 1), ("drop", 3)),
]


def _drop(dc, dropped):
    """dc with the blocks at the (iblock, jblock) positions `dropped` eliminated, local indices renumbered"""
    for b in dc.blocks:
        if (b.iblock, b.jblock) in dropped:
            b.owner = -1
    for r in range(dc.nranks):
        for k, b in enumerate(sorted((b for b in dc.blocks if b.owner == r), key=lambda b: b.gid)):
            b.local = k
    return dc


def _all_dims(dc):
    return [evp.make_dims(dc, rank) for rank in range(dc.nranks)]


# ---- the refusals: a good description with one thing wrong ----
def _nghost2():
    d, keep = evp.make_dims(decomp.single_block(24, 16, "cyclic", "closed"))
    d.nghost = 2
    return [(d, keep)]


def _no_table():
    out = _all_dims(decomp.per_rank_blocks(48, 20, 2, "cyclic", "closed", (2, 1)))
    for d, keep in out:
        d.nblocks_tot = 0
    return out


def _count_disagrees():
    out = _all_dims(decomp.Decomp(72, 40, 18, 10, "cyclic", "closed", 2, (2, 1)))
    for d, keep in out:
        d.nblocks -= 1
    return out


def _origin_disagrees():
    out = _all_dims(decomp.Decomp(72, 40, 18, 10, "cyclic", "closed", 2, (2, 1)))
    for d, keep in out:
        d.iglob0[1] += 1                # the second local block
    return out


REFUSALS = {
    "refuse-nghost2": (_nghost2, "halo plan: nghost must be 1 (ice_blocks.F90:47)"),
    "refuse-no_table": (_no_table, "halo plan: global block table required when nranks > 1"),
    "refuse-count": (_count_disagrees, "halo plan: global block table disagrees with nblocks of this rank"),
    "refuse-origin": (_origin_disagrees, "halo plan: local block geometry inconsistent with the global block table"),
}


def _cases():
    """name -> a function that gives (Dims, keepalive) of every rank"""
    c = {}
    for ew in EW:                       # boundary kinds, one block, one rank (tripole / tripoleT without a cyclic ew: refused)
        for ns in NS:
            c["one-%s-%s" % (ew, ns)] = lambda ew=ew, ns=ns: _all_dims(decomp.single_block(24, 16, ew, ns))
    for ns in ("tripole", "tripoleT"):  # odd nx_global: refused
        c["one-odd-%s" % ns] = lambda ns=ns: _all_dims(decomp.single_block(23, 16, "cyclic", ns))
    for ns in NS:                       # several blocks on one rank; 70 x 38: the last block padded both ways, column NX/2 inside a block
        c["blocks-72x40-%s" % ns] = lambda ns=ns: _all_dims(decomp.Decomp(72, 40, 18, 10, "cyclic", ns, 1))
        c["blocks-70x38-%s" % ns] = lambda ns=ns: _all_dims(decomp.Decomp(70, 38, 18, 10, "cyclic", ns, 1))
    for k, case in enumerate(HALO_CASES):
        c["cgfold-%02d-%s" % (k, case[4])] = lambda case=case: _all_dims(fold_cases._layout(case))
    for px, py in SPLIT_SHAPES:
        c["split-%dx%d" % (px, py)] = lambda s=(px, py): _all_dims(decomp.per_rank_blocks(48, 20, s[0] * s[1], "cyclic", "tripole", s))
    for ew, ns in (("cyclic", "closed"), ("closed", "closed"), ("cyclic", "cyclic")):
        for px, py in ((2, 1), (1, 2), (2, 2)):
            c["ranks-%s-%s-%dx%d" % (ew, ns, px, py)] = lambda ew=ew, ns=ns, s=(px, py): _all_dims(
                decomp.per_rank_blocks(48, 20, s[0] * s[1], ew, ns, s))
    for ns in ("tripole", "tripoleT"):  # eliminated land blocks: 4 x 4 blocks on two ranks
        # a block of a lower block row: zero fill away from the fold
        c["land-low-%s" % ns] = lambda ns=ns: _all_dims(_drop(decomp.Decomp(72, 40, 18, 10, "cyclic", ns, 2, (2, 1)), {(2, 2)}))
        # the two middle blocks of the top row, each other's fold partners: pairs with neither half (b = -2 with a = -1)
        c["land-partners-%s" % ns] = lambda ns=ns: _all_dims(_drop(decomp.Decomp(72, 40, 18, 10, "cyclic", ns, 2, (2, 1)), {(2, 4), (3, 4)}))
    for name, (make, text) in REFUSALS.items():
        c[name] = make
    return c


CASES = _cases()


def _last_error():
    buf = C.create_string_buffer(1024)
    evp.load_library(testing=True).cice_evp_hip_last_error(buf, 1024)
    return buf.value.decode()


def plan_digest(ranks):
    """one digest over the dumps of all ranks, in rank order; a refused rank contributes the library's error text"""
    h = hashlib.sha256()
    for d, keep in ranks:
        try:
            h.update(evp.halo_plan_dump(d).tobytes())
        except evp.EvpHipError:
            h.update(b"refused:" + _last_error().encode())
    return h.hexdigest()


DIGESTS = {
    "blocks-70x38-closed": "b175161f5b8a0dc836c65da43096c90bab0efdac799ea13742bac61855144310",
    "blocks-70x38-cyclic": "02f7fff866bcb8981d1cf3b935b6fcca9ad5600bf9f9a648cc06a619da1fa28b",
    "blocks-70x38-open": "b175161f5b8a0dc836c65da43096c90bab0efdac799ea13742bac61855144310",
    "blocks-70x38-tripole": "f3032f241bbc52b27624c0101818614652908eb1ecfca92de8d0b4cb6a3b0104",
    "blocks-70x38-tripoleT": "7ffff8ded39ba66d07fde6b8eb5d991af794466c2e48ef5a318407cc55aed7af",
    "blocks-72x40-closed": "5648876fb74934a08404e043867be0e14c0c239fdcc2fb2677b39410f9c7f528",
    "blocks-72x40-cyclic": "e2287c24bb2c3b86ecac5a884f84bbb9f7453a2127efdfa010f8aab70ed14efc",
    "blocks-72x40-open": "5648876fb74934a08404e043867be0e14c0c239fdcc2fb2677b39410f9c7f528",
    "blocks-72x40-tripole": "068d04a8af77723e2798c6ddd27d5a4f78c77076d0069dafecd3ec4f29a94168",
    "blocks-72x40-tripoleT": "ee2ac8787f9f9ec90d62221ef25e1d06bd255f14e65a6792bdb4dde864e1f7e4",
    "cgfold-00-tripole": "c50b07e603b1d3c2a400b197d83d9d9218b8c72e95a261c79618263dfe6a3d68",
    "cgfold-01-tripole": "9b9882599dcdcd80388f03b5c44eeba41ed2e3d6033da11c89723f11d89871f2",
    "cgfold-02-tripole": "61b1c92425e0082e4d325b592d06d907a2d5e6780a81b097602611150990a07f",
    "cgfold-03-tripole": "d8ac59ed68f8c381a825977663c49c1987750464632ab011aa619594d43bd938",
    "cgfold-04-tripole": "580cf09809b8d1d64cea374a17c686ca05368cdb4f27aa9f79876d11bc9dde91",
    "cgfold-05-tripole": "ecdc33ae622af3fac8ae7bca5660542eac2e39c32e8f910d230a3fd16f7feac5",
    "cgfold-06-tripoleT": "9e4427c3d4329ddfb0d60ae922349904d0b599d2fe0420464aaeb8a9271bf1e6",
    "cgfold-07-tripoleT": "5a9da7a2134b9e14339148f09b8a708d227183443901735d0c367662e152f171",
    "cgfold-08-tripoleT": "917160f9d1e165dfea8be96df37c3acc654ceedd61203e0f89862eaecb490152",
    "cgfold-09-tripoleT": "5dcda0b21240477823bfadf7ec9f063e3a5b9298d4542190ca9ae1ff82f838a7",
    "cgfold-10-tripoleT": "d04d0893ea57830ef7d550678b0dee89d21e63dea0948b230b9ab63960b03945",
    "cgfold-11-tripoleT": "0fc7a3c0b03c695cb8db0fc5759bd7eae24b35e90cc5780649375eb5da2c2a15",
    "land-low-tripole": "043ca078f0982c2930abf421e0d455e836bdb12611ade545b934f25f23cd0b22",
    "land-low-tripoleT": "387b96a93e51d104012e1d224569f4bdb4c557f313c88a2f0ae6716a7b609ed2",
    "land-partners-tripole": "39a3ee4ee7f5cbb1548e96b62c7119fe32922e1c66f46852ef7f90154dd27df5",
    "land-partners-tripoleT": "290e566d9b46b286aeab22a6f3bacf27e74d02094184b18c2fb5d40fd115b506",
    "one-closed-closed": "f40e269fcd50453b786fe90c758a4e1f826bd0e9f4ebf8b209601fadf14d3aea",
    "one-closed-cyclic": "ea7cfed58e3bea3fbdd3b0dbaff02636d5cb7ab04b64606828b218d84552b4a9",
    "one-closed-open": "f40e269fcd50453b786fe90c758a4e1f826bd0e9f4ebf8b209601fadf14d3aea",
    "one-closed-tripole": "9e61372b1882f1e6f874cb81d0e8ee51d2cb31a92faa788fd1928db68d492330",
    "one-closed-tripoleT": "9e61372b1882f1e6f874cb81d0e8ee51d2cb31a92faa788fd1928db68d492330",
    "one-cyclic-closed": "295711147aa8ac83169f454b05a93914255d62ae1a1a8ef2bc29f3e3c1d6682b",
    "one-cyclic-cyclic": "72b347f3a2c094afef33450822c52d8af41e97014ad855cbfe3d39f6863832b5",
    "one-cyclic-open": "295711147aa8ac83169f454b05a93914255d62ae1a1a8ef2bc29f3e3c1d6682b",
    "one-cyclic-tripole": "a704b87c2c18ff8b6c2558293538922388663f6c864ab263b3209e3b80265b9b",
    "one-cyclic-tripoleT": "4f03da698b2e396fc39c74d84930de58e7565ed85b90b7769f544ab2a15a95e6",
    "one-odd-tripole": "9e61372b1882f1e6f874cb81d0e8ee51d2cb31a92faa788fd1928db68d492330",
    "one-odd-tripoleT": "9e61372b1882f1e6f874cb81d0e8ee51d2cb31a92faa788fd1928db68d492330",
    "one-open-closed": "f40e269fcd50453b786fe90c758a4e1f826bd0e9f4ebf8b209601fadf14d3aea",
    "one-open-cyclic": "ea7cfed58e3bea3fbdd3b0dbaff02636d5cb7ab04b64606828b218d84552b4a9",
    "one-open-open": "f40e269fcd50453b786fe90c758a4e1f826bd0e9f4ebf8b209601fadf14d3aea",
    "one-open-tripole": "9e61372b1882f1e6f874cb81d0e8ee51d2cb31a92faa788fd1928db68d492330",
    "one-open-tripoleT": "9e61372b1882f1e6f874cb81d0e8ee51d2cb31a92faa788fd1928db68d492330",
    "ranks-closed-closed-1x2": "4e843cf94f1625bdad55cbda4da45829740891dedde70af313ae003763555d47",
    "ranks-closed-closed-2x1": "830d35dce3609b7bd4a45035a5f33465245fee0dc79f6c8c0e0ba3482ed3807b",
    "ranks-closed-closed-2x2": "cca995a5e1f9ceef7d0edebbf2419eb373cf1e83af294ca9f86257e0ddab179e",
    "ranks-cyclic-closed-1x2": "5e1005804f02ea381911fbc4fef0ba96bfda452dfb3828826ad750daf5a36f01",
    "ranks-cyclic-closed-2x1": "3ac34537aa0ad62404839198843cc1ef2459aba4446b4e461c4c7edda0cce642",
    "ranks-cyclic-closed-2x2": "a9798701fb4b88ba3108c23a2e4e455c0509c273d6a98a6ba501588e3dbfec83",
    "ranks-cyclic-cyclic-1x2": "6586a5f589ab7c707603783bf9e4f4cdae31588102b3dd15e58425802b5ab8e6",
    "ranks-cyclic-cyclic-2x1": "72d5293a2ffbfada58c4375001bc12b303b7f06e9b86f0ecfbad43de2b60b569",
    "ranks-cyclic-cyclic-2x2": "e6bf69067f677075923459814db5a9038b1354ca9c71c26e7deabbad372f0a1f",
    "refuse-count": "dc937befc6b873091a117dfb7fa6d4eff9c05c9d0d411f73441492bcbf836c6c",
    "refuse-nghost2": "1a74cad0cdf0c5af818aabef9a229403bc679e60c99278c28d3f5e2a6e273382",
    "refuse-no_table": "c53ab0bf5eddf71b17d048b55cd87752c6933b1d29a390b630cc5a5db78885ec",
    "refuse-origin": "76a52247d9b018c250285dbae02036db066f940ccda1ecbee98279917dcf9a53",
    "split-2x1": "026129e9fa226e7f7c10343635997ded131289a518e32b811af1e78e536cdddd",
    "split-2x2": "c28a44c0813cba193a5463062907d5c7fe3c677e63be78a202d2daa773413167",
    "split-3x1": "302b8dfd800016b4ba908024d16e2875ed7b8aa7808ea8cf0cb35cc0902374bd",
    "split-4x1": "09999d32999282d0764390db3c3d5aacad5c299aed9f6bf232d87242806ce2e7",
    "split-4x2": "ee0976953653dd8d6418b15aae96d0646d8ef4e9f35a40ac14b66ddb800ad192",
}


def test_the_cases_are_those_the_digests_were_recorded_for():
    assert fold_cases.HALO_CASES == HALO_CASES
    marks = [m for m in multirank_cases.test_fold_row_split_over_ranks_lists_of_the_on_chip_kernel.pytestmark if m.name == "parametrize"]
    assert [tuple(s) for s in marks[0].args[1]] == SPLIT_SHAPES
    assert tuple(sorted(evp.BND, key=evp.BND.get)) == NS and set(EW) <= set(NS)
    assert sorted(DIGESTS) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_halo_plan_bytes_are_the_recorded_ones(case):
    assert plan_digest(CASES[case]()) == DIGESTS[case]


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusal_text(case):
    make, text = REFUSALS[case]
    for d, keep in make():
        with pytest.raises(evp.EvpHipError):
            evp.halo_plan_dump(d)
        assert _last_error() == text
