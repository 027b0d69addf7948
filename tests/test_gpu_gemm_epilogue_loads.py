"""The epilogue forms of the 1x1-conv GEMMs that read an auxiliary operand -- residual (ctn_pw_gemm with a residual, with and without
the gLN prologue), ctn_pw_dgrad_gln and ctn_pw_dgrad_cln -- at the shapes that reach every path of gemm_epilogue's pass loop
(csrc/ctn_gemm_common.h): the auxiliary loads of a 32-row group are issued in one batch ahead of the group's stores, and the predicate
of a column tile that overhangs Kp is taken once per thread, outside the loop.

Shapes, the smallest that reach every path:
    M = 2, Cn = 64
    R = 96, 160     no multiple of the 128- and 256-row tiles: rows >= R are dropped by the range check; 96 runs one 128x64 tile (and
                    two 64x64 tiles under fp32 arithmetic), 160 the 256x64 tile of the residual-on-pieces forms and two 128x64 row tiles
    K = 61,  Kp = 64    one full column tile, frames >= K
    K = 130, Kp = 132   two full column tiles and one that overhangs Kp: of each wave's 16 lanes per staged row one is live
                        (columns 128 .. 131) and fifteen are masked out by the hoisted predicate
    and, at R = 160, K = 130, the 256x64 tile on four waves (ctn_tune("b3_tile" / "b3_tile_k3", 2)): two row groups per wave, so the
    second group's batch is issued before the first group's stores.

Every case goes through test_gpu_gemm_seams.check, which is what that module applies to these forms: outputs pre-filled with NaN between
4096 sentinel elements on either side -- afterwards no sentinel is touched and no NaN is left (nothing outside the [R, Kp) matrices of
the M utterances was written, everything inside was); a second call gives the same bits, outputs and partials; utterance m of the M = 2
call is bitwise the M = 1 call; out_amax is bitwise max |Out[m]|; and against tests/gemm_oracle.py in fp64 with that module's limits
(gemm_oracle.LIMIT): 3e-6 / 5e-6 of max |ref| for Out / dN, 6e-7 of sum |a||b| (or 1.25x the fp32 MFMA's error) for the h3 entry
points, 1e-5 of the sum of the terms' absolute values for every statistics partial, 2e-5 for the cLN backward's per-frame constants.
"""
import pytest

import gemm_oracle as GO
import test_gpu_gemm_seams as S
from conftest import ARITH

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]

CN = 64
SHAPES = [(R, K, Kp) for R in (96, 160) for K, Kp in ((61, 64), (130, 132))]
FORMS = ("res", "k3", "b1", "clnb")


@pytest.fixture(autouse=True)
def _own_references():
    print()
    yield
    S._REF.clear()          # a reference is shared among the weight forms of one test, not kept beyond it


def weight_forms(form, pieces_only=False):
    """The stored weight (the family that the arithmetic selects), b6 pieces under the split arithmetics, h3 pieces under all three."""
    wfs = [] if pieces_only else ["w1" if form in S.DGRAD_FORMS else "w0"]
    if ARITH["name"] != "fp32":
        wfs.append("b6")
    return wfs + ["h3"]


@pytest.mark.parametrize("R,K,Kp", SHAPES, ids=["R%d-K%d-Kp%d" % s for s in SHAPES])
def test_auxiliary_load_forms_default_tiles(R, K, Kp):
    c = S.Case(GO.make_inputs(R, CN, K, Kp))
    assert c.i.M == 2 and c.i.Kp == Kp
    fam = GO.family_of(ARITH["name"], R)
    S.assert_parts(R, Kp, GO.tile_of(fam, GO.DEFAULT_TILE[fam]), fam)
    for form in FORMS:
        for wf in weight_forms(form):
            tile_fam = "split" if wf == "h3" else fam
            S.check("epilogue loads", form, wf, c, GO.tile_of(tile_fam, GO.DEFAULT_TILE[tile_fam]))


def test_auxiliary_load_forms_two_row_groups_per_wave():
    """256x64 tile on four waves: each wave owns 64 rows = two 32-row groups (two register sets of auxiliary loads)."""
    R, K, Kp = 160, 130, 132
    tile = GO.B3_TILES[2]
    assert tile == (256, 64)
    c = S.Case(GO.make_inputs(R, CN, K, Kp))
    with S.tuned(b3_tile=2, b3_tile_k3=2):
        S.assert_parts(R, Kp, tile, "split")
        for form in FORMS:
            for wf in weight_forms(form, pieces_only=True):
                S.check("epilogue loads, 2 groups", form, wf, c, tile)
