"""The two C-grid zone / rest plans (cice_amd/csrc/halo_plan.cpp: build_cg_frame, build_cg_march_fold), byte for byte: a SHA-256 over
everything the test build's cice_evp_hip_cgrid_frame_plan and cice_evp_hip_cgrid_march_fold_plan hand out -- the cells' bytes, every
workgroup list, the items, every info value, and the reason where a plan declines -- for every rank of every case of
test_cgrid_frame_plan_cpu.py and every parametrisation of test_cgrid_march_fold_plan_cpu.py.

The expected digests were recorded from the library of the commit BEFORE the two planners were put on one split helper and one table
of reads each, with this file's own digest functions; they pin that the rewrite changed no byte of any plan.  Those two files restate
the stencils in numpy and stay the independent check of what the bytes mean; this one only says "as before".  A deliberate change of
a plan (a new level, another stencil) re-records the literals it changes, and says so.
"""
import hashlib

import numpy as np
import pytest

from cice_amd import decomp, evp

import test_cgrid_frame_plan_cpu as frame_cases
import test_cgrid_march_fold_plan_cpu as fold_cases


def _digest(plan, keys):
    h = hashlib.sha256()
    if plan is None or "declined" in plan:
        h.update(b"declined:" + (b"" if plan is None else plan["declined"].encode()))
        return h.hexdigest()
    h.update(np.ascontiguousarray(plan["cells"], dtype=np.uint8).tobytes())
    h.update(np.int64(len(plan["wg"])).tobytes())
    for wg in plan["wg"]:
        h.update(np.int64(len(wg)).tobytes())
        h.update(np.ascontiguousarray(wg, dtype=np.int32).tobytes())
    h.update(np.ascontiguousarray(plan["items"], dtype=np.int32).tobytes())
    h.update(np.asarray([int(plan[k]) for k in keys] + [len(plan["items"])], dtype=np.int64).tobytes())
    return h.hexdigest()


def frame_digest(dc, world):
    """one digest over the plans of all ranks, in rank order"""
    h = hashlib.sha256()
    for rank in range(world):
        d, keep = evp.make_dims(dc, rank)
        h.update(_digest(evp.cgrid_frame_plan(d), ("zone_cells", "frame_cells")).encode())
    return h.hexdigest()


def fold_digest(dc, world=1, **kw):
    h = hashlib.sha256()
    for rank in range(world):
        d, keep = evp.make_dims(dc, rank)
        h.update(_digest(evp.cgrid_march_fold_plan(d, **kw), ("zone_cells", "rest_cells", "fold_band_rows", "segment_rows", "lengths")).encode())
    return h.hexdigest()


FRAME = {
    "cut1x2": "18e35861fa2397f8c9e22db207a308164ca47deac3ba5a2c3d75bc096f60fff0",
    "cut2x1": "effa23ae0236554b25b60d1c21525129285f851644d894bb2c3eeaf6ffff0116",
    "cut2x1_blocks2x2": "199ad912df76fe2f307783656201149b814b33aa0667707861feb834dc4cfb8b",
    "cut2x2": "68571d7cebb81279de9d26f68ce2a85dc787447c53a58d1663b6cce56978d715",
    "cut2x2_blocks2x2": "d12bd1fe7cbacdefe83f8d936a353eebc817bcc9f45729c9c2d6bad1ecf6835c",
    "cut3x1": "3f5005e1ec37c9eed78bfd7a9d0fff1773847bf1063ba760920012137fbdf803",
    "no_zone": "3296d72534ec12188345456979f7b3b74b03a548307555e0d1ac6c8d2d0f18f1",
    "rows56": "397824cd1e9e7ecca5197f916eb5f4ebecceaa770d4b12e80c19c6bbd70170bb",
    "rows61": "fe670e543672b6697257786eb3a01f06cb3407244b9e6811c509f6d026cfdc6f",
    "rows121": "881d821a91c005cedf140f29a58ab0a4e7ab21c4e030d849c2f8fae2fa434750",
    "rows216": "24aa6944a5d33d15da6eca5414e242768702e4f318cd8e2ecf5fe295b519f96d",
    "one_rank": "755e40d57412ea815723c20bf221693bb96c86d3372c564356fae59bdcb01a3a",
}

FOLD = {
    "100x116_1blk-tripole-1": "47063d845288b1b7c8b3d4e53297afc845b53df123e4f22928603613208bcaaf",
    "100x116_1blk-tripole-0": "dfab33f40a5074c90d8e5c88fb5a83f310072e6ea0e60efd086657a48163dbee",
    "100x116_1blk-tripoleT-1": "47063d845288b1b7c8b3d4e53297afc845b53df123e4f22928603613208bcaaf",
    "100x116_1blk-tripoleT-0": "dfab33f40a5074c90d8e5c88fb5a83f310072e6ea0e60efd086657a48163dbee",
    "200x64_1blk-tripole-1": "c5323b6a1cc229c51476b5651bce2a8d04f117d82beb7f309c8bdf67e6e8ac0d",
    "200x64_1blk-tripole-0": "325d77e8ed13c5928d7b49fd35ca9d11c04d9b1c6a5cabae57da24159a9a746a",
    "200x64_1blk-tripoleT-1": "c5323b6a1cc229c51476b5651bce2a8d04f117d82beb7f309c8bdf67e6e8ac0d",
    "200x64_1blk-tripoleT-0": "325d77e8ed13c5928d7b49fd35ca9d11c04d9b1c6a5cabae57da24159a9a746a",
    "260x72_140x40pad-tripole-1": "056846a84f40b2f6ad102c652dc9deceb68cc5279fb81aa21ecc64e4fc8d3e7d",
    "260x72_140x40pad-tripole-0": "1a4be62d20d34f6d7805159de36f3fa6ebb6d5d6728451ad94e5b091a1ca13f5",
    "260x72_140x40pad-tripoleT-1": "b6068189148533f03af93da7a021977231ab6d3baa9493be56c9381308cb75ed",
    "260x72_140x40pad-tripoleT-0": "a4e53b64f0cd7aa773c35b6e524a8b4a833ab6d1442d29c123424ffa92091b7d",
    "260x72_90x30pad-tripole-1": "2b339712e146908d3a8dd12ee2d818e7878955e1bffd33e2fc698edceb28a3f4",
    "260x72_90x30pad-tripole-0": "42d7875e802889753318d8988a83d428777d3467b213717062d30a06dcbbcfad",
    "260x72_90x30pad-tripoleT-1": "c319da773419eac58cd317c5b57d13f9c454cec454463ccd6d8b3a0c446f3e01",
    "260x72_90x30pad-tripoleT-0": "85224e7e91c2c8da09f6f2aabd77270bfa02a3864577668992c13a7ac8962906",
    "400x80_200x40-tripole-1": "3cafc992016ea572e7f400ad57d0db5b38c944020241b5bb55b483d7f257b962",
    "400x80_200x40-tripole-0": "e517029cf17bc80fa964160c38d98cb12712a72439b57b7bbe51a32055e75ce8",
    "400x80_200x40-tripoleT-1": "3cafc992016ea572e7f400ad57d0db5b38c944020241b5bb55b483d7f257b962",
    "400x80_200x40-tripoleT-0": "e517029cf17bc80fa964160c38d98cb12712a72439b57b7bbe51a32055e75ce8",
    "closed": "3d5f1f3150edaaca08ecedeef3bf580a1029e4cd3e592b230a9b54c9069d8910",
    "two_ranks": "1fd57cbda2984aabe0ba201e96b441508c7b78fa9c6ea0aa06d0aa38a6f3ac36",
    "too_short-tripole": "3390c154da0ff047e0469e93c8897a47a556b6bd5040d6c8b70519d80155e51c",
    "too_short-tripoleT": "3390c154da0ff047e0469e93c8897a47a556b6bd5040d6c8b70519d80155e51c",
}


def _frame_case(case):
    if case == "one_rank":                      # declines: no neighbour on another rank
        return decomp.single_block(400, 216, "cyclic", "closed"), 1
    if case.startswith("rows"):
        return frame_cases._decomp(300, int(case[4:]), (2, 1), None)
    nx, ny, shape, bpr = frame_cases.CASES[case]
    return frame_cases._decomp(nx, ny, shape, bpr)


def test_the_cases_are_those_of_the_two_plan_tests():
    rows = ["rows%d" % (5 * k + 6) for k in (10, 11, 23, 42)]
    assert sorted(FRAME) == sorted(list(frame_cases.CASES) + rows + ["one_rank"])
    grids = ["%s-%s-%d" % (g, ns, ln) for g in fold_cases.GRIDS for ns in ("tripole", "tripoleT") for ln in (1, 0)]
    assert sorted(FOLD) == sorted(grids + ["closed", "two_ranks", "too_short-tripole", "too_short-tripoleT"])


@pytest.mark.parametrize("case", sorted(FRAME))
def test_frame_plan_bytes_are_the_recorded_ones(case):
    dc, world = _frame_case(case)
    assert frame_digest(dc, world) == FRAME[case]


@pytest.mark.parametrize("case", sorted(FOLD))
def test_march_fold_plan_bytes_are_the_recorded_ones(case):
    if case == "closed":                        # declines: no tripole fold
        got = fold_digest(decomp.single_block(400, 216, "cyclic", "closed"))
    elif case == "two_ranks":                   # declines: several ranks
        got = fold_digest(decomp.per_rank_blocks(400, 216, 2, "cyclic", "tripole", proc_shape=(1, 2)), world=2)
    elif case.startswith("too_short"):          # declines: no rectangle left under the band
        got = fold_digest(decomp.single_block(200, 10, "cyclic", case.split("-")[1]))
    else:
        grid, ns, lengths = case.split("-")
        nx, ny, bs = fold_cases.GRIDS[grid]
        got = fold_digest(fold_cases._decomp(nx, ny, bs, ns), lengths=int(lengths))
    assert got == FOLD[case]
