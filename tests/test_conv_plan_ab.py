"""The launch plan of the dual-gate epilogue (csrc/conv_plan.h conv_plan with ConvAsk::dual_mul, through lrp_conv_plan and
LRP_PLAN_DUAL_MUL): which form and tile every reverse launch of the alpha-beta walk (beta > 0) takes, what the plan refuses for
it, and that the operator table tests/conv_ab_cases.py reaches every form it can answer.  Pure host arithmetic: no GPU."""
import pytest

import conv_ab_cases as T
from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.engine import conv_plan, switches
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG

MUL, UP2, FP, BF, DM = K.LRP_EPI_MUL, K.LRP_EPI_MUL_UP2, K.LRP_OPND_FP32, K.LRP_OPND_BF16X3, K.LRP_PLAN_DUAL_MUL
TINY = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, False), ("c4", 16, 16, True), ("c5", 16, 16, False)]
MID = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, True), ("c4", 128, 256, False), ("c5", 256, 128, False)]
WIDE = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, False), ("c4", 128, 128, True), ("c5", 128, 256, False),
        ("c6", 256, 512, True), ("c7", 512, 512, False)]
RESIDENT_SET = {"LRP_CONV_SMALL": 0, "LRP_CONV_MID": 0, "LRP_CONV_HALO": 2}


def walk(cfg, hw, n, prec):
    """the plans of the reverse launches through convs 1 .. top of `cfg` over n relevance maps, as names, top first"""
    H, dims = hw, []
    for i, (_, cin, cout, pool) in enumerate(cfg):
        dims.append((cin, cout, H, i > 0 and cfg[i - 1][3]))
        H = H // 2 if pool else H
    out = []
    for cin, cout, H, pooled in reversed(dims[1:]):
        p = conv_plan(UP2 if pooled else MUL, prec, n, H, H, cin, 2 * cout, flags=DM)
        assert p["ok"] == 1
        out.append(T.plan_name(p))
    return out


def test_small_walks_take_the_staged_tiles():
    for prec in (FP, BF):
        assert walk(TINY, 16, 6, prec) == ["PLAIN 128x32"] * 4
        assert walk(MID, 32, 4, prec) == ["SMALL 64x64"] * 4
        assert walk(WIDE, 32, 4, prec) == ["SMALL 64x64"] * 6


def test_small_walks_under_the_resident_image_switch_set():
    with switches(**RESIDENT_SET):
        assert walk(TINY, 16, 6, BF) == ["PLAIN 128x32"] * 4
        assert walk(MID, 32, 4, BF) == ["HALO 128x128 tw8 th9"] * 2 + ["PLAIN 128x64"] * 2
        assert walk(WIDE, 32, 4, BF) == ["HALO 128x128 tw4 th8"] + ["HALO 128x128 tw8 th9"] * 3 + ["PLAIN 128x64"] * 2
        assert walk(MID, 32, 4, FP) == ["PLAIN 128x64"] * 4            # (exact fp32 has no resident-image kernel)


def test_vgg16_walks():
    # 3 tokens: small grids.  320 tokens: the pipelined resident-image tile from block2_conv2 up in split-bf16 — never the
    # 8-wave tile, which the single-gate walk takes for N % 256 == 0 at this size — and the staged tiles in exact fp32
    assert walk(VGG16_CFG, 224, 3, BF) == (["SMALL 64x64"] * 6 + ["PLAIN 128x64"] * 2 + ["SMALL 64x64", "HALO 128x128 tw14 th9"]
                                           + ["PLAIN 128x64"] * 2)
    assert walk(VGG16_CFG, 224, 3, FP) == (["SMALL 64x64"] * 3 + ["PLAIN 128x64"] * 2 + ["SMALL 64x64"] + ["PLAIN 128x64"] * 6)
    assert walk(VGG16_CFG, 224, 320, BF) == ["HALO 128x128 tw14 th9"] * 10 + ["PLAIN 128x64"] * 2
    assert walk(VGG16_CFG, 224, 320, FP) == ["PLAIN 128x64"] * 3 + ["PLAIN 128x128"] * 7 + ["PLAIN 128x64"] * 2
    single = conv_plan(MUL, BF, 320, 28, 28, 512, 512, flags=K.LRP_PLAN_FRAG)
    assert (single["BM"], single["BN"]) == (256, 256)
    dual = conv_plan(MUL, BF, 320, 28, 28, 512, 1024, flags=DM)
    assert (dual["form"], dual["BM"], dual["BN"], dual["threads"]) == (K.LRP_FORM_HALO, 128, 128, 256)


def test_every_answer_is_a_form_the_dual_gate_is_built_for():
    allowed = {("PLAIN", 128, 128), ("PLAIN", 128, 64), ("PLAIN", 128, 32), ("SMALL", 64, 64), ("HALO", 128, 128)}
    sets = ({}, {"LRP_CONV_SMALL": 0}, {"LRP_CONV_SMALL": 0, "LRP_CONV_MID": 0}, RESIDENT_SET, {"LRP_CONV_HALO": 0},
            {"LRP_CONV_HALO": 2}, {"LRP_CONV_BREG": 0}, {"LRP_CONV_BREG8": 0, "LRP_CONV_BREG4": 0})
    for sw in sets:
        with switches(**sw):
            for prec in (FP, BF):
                for epi in (MUL, UP2):
                    for NB, H in ((1, 14), (3, 14), (2, 28), (33, 56), (320, 14), (320, 28), (64, 112)):
                        for N, C in ((8, 8), (24, 16), (64, 64), (72, 136), (128, 64), (256, 256), (512, 512)):
                            p = conv_plan(epi, prec, NB, H, H, N, 2 * C, flags=DM)
                            assert p["ok"] == 1, (sw, prec, epi, NB, H, N, C)
                            assert (T.FORM_NAMES[p["form"]], p["BM"], p["BN"]) in allowed, (sw, T.plan_name(p))
                            assert p["threads"] == 256
                            if T.FORM_NAMES[p["form"]] == "HALO":
                                assert prec == BF


def test_what_the_plan_refuses():
    ok = conv_plan(MUL, BF, 3, 14, 14, 128, 256, flags=DM)
    assert ok["ok"] == 1
    for extra in (K.LRP_PLAN_UP2_SRC, K.LRP_PLAN_IMG_PART, K.LRP_PLAN_POOL_GC, K.LRP_PLAN_FRAG, K.LRP_PLAN_JOIN, K.LRP_PLAN_GMASK):
        for prec in (FP, BF):
            for epi in (MUL, UP2):
                assert conv_plan(epi, prec, 3, 14, 14, 128, 256, flags=DM | extra)["ok"] == 0, extra
    # the frag forms at the sizes where the single-gate launch takes them: N = 64 (BREG), N % 128 (BREG4), N % 256 at 320 tokens (BREG8)
    for NB, H, N, C in ((2, 28, 64, 64), (320, 28, 128, 128), (320, 28, 512, 512)):
        assert conv_plan(MUL, BF, NB, H, H, N, C, flags=K.LRP_PLAN_FRAG)["ok"] == 1
        assert conv_plan(MUL, BF, NB, H, H, N, 2 * C, flags=DM | K.LRP_PLAN_FRAG)["ok"] == 0
    # fp16 pairs, the two-MFMA forms, the other epilogues
    assert conv_plan(MUL, K.LRP_OPND_F16X2, 3, 14, 14, 128, 256, flags=DM)["ok"] == 0
    assert conv_plan(MUL, K.LRP_OPND_F16X2, 3, 14, 14, 128, 256, terms=5, flags=DM)["ok"] == 0
    for epi in (K.LRP_EPI_BIAS, K.LRP_EPI_BIAS_RELU, K.LRP_EPI_STORE, K.LRP_EPI_IMG_STENCIL):
        assert conv_plan(epi, FP, 3, 14, 14, 128, 256, flags=DM)["ok"] == 0
    assert conv_plan(K.LRP_EPI_FWD_DUAL, FP, 3, 14, 14, 256, 128, split=128, flags=DM)["ok"] == 0
    # a chain must be whole groups: 2 C % 16 (split) / % 8 (fp32)
    assert conv_plan(MUL, BF, 3, 14, 14, 128, 24, flags=DM)["ok"] == 0
    assert conv_plan(MUL, BF, 3, 14, 14, 128, 48, flags=DM)["ok"] == 1
    assert conv_plan(MUL, FP, 3, 14, 14, 128, 12, flags=DM)["ok"] == 0
    assert conv_plan(MUL, FP, 3, 14, 14, 128, 24, flags=DM)["ok"] == 1
    # ... and the output columns whole 16 B / 32 B groups, as for the single gate
    assert conv_plan(MUL, BF, 3, 14, 14, 12, 32, flags=DM)["ok"] == 0
    assert conv_plan(MUL, FP, 3, 14, 14, 6, 32, flags=DM)["ok"] == 0


def test_without_the_flag_nothing_changes():
    for sw in ({}, RESIDENT_SET):
        with switches(**sw):
            for NB, H, N, C in ((3, 14, 128, 256), (320, 28, 512, 512), (2, 28, 64, 64)):
                for flags in (0, K.LRP_PLAN_FRAG):
                    a = conv_plan(MUL, BF, NB, H, H, N, C, flags=flags)
                    assert a["ok"] == 1


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_gets_its_plan(case):
    with switches(**case.switches):
        for pool in (False, True):
            p = T.op_plan(case, pool)
            assert p["ok"] == 1
            assert (T.FORM_NAMES[p["form"]], (p["BM"], p["BN"])) == (case.form, tuple(case.tile)), (T.plan_name(p), pool)
    if case.split:
        assert 9 * case.Cout >= T.MIN_SPLIT_K


def test_table_reaches_every_form():
    assert T.uncovered(T.CASES) == []
    assert T.uncovered(T.CASES[1:]) != []                     # (the check can fail)
