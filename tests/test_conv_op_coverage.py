"""The operator cases of tests/conv_cases.py against the launch plan (csrc/conv_plan.h conv_plan, through lrp_conv_plan): every
case takes the form and tile it states under its switches, and together the cases reach every (operand format, epilogue, form,
tile) that lrp_op_conv can take — so a change of the plan that moves a case onto another kernel, or a case that is dropped,
shows here and not as a silent loss of what tests/test_gpu_conv_forms.py compares with float64.  Host arithmetic only — no GPU."""
import pytest

import conv_cases as T
from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.build import build_library
from lrp_imagecaptioning_amd.engine import conv_plan, switches


@pytest.fixture(scope="module", autouse=True)
def _library():
    build_library()


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_takes_the_plan_it_states(case):
    with switches(**case.switches):
        p = T.op_plan(case)
    assert p["ok"] == 1, p
    assert (T.FORM_NAMES[p["form"]], (p["BM"], p["BN"])) == (case.form, tuple(case.tile)), (T.plan_name(p), case)
    assert p["threads"] == (512 if p["BM"] == 256 else 256)
    assert (p["tw"] > 0) == (case.form in T.RESIDENT), p


def test_split_cases_stay_where_the_element_bar_is_derived():
    for c in T.CASES:
        if c.split:
            assert c.taps * T.launch_dims(c)[0] >= T.MIN_SPLIT_K, T.case_id(c)


def test_case_ids_are_unique():
    ids = [T.case_id(c) for c in T.CASES]
    assert len(set(ids)) == len(ids)


def test_the_table_reaches_every_form_of_the_operator():
    assert T.uncovered(T.CASES) == []


def test_a_dropped_case_is_named():
    """removing the only case of a form fails the coverage check with that (format, epilogue, form, tile) in the message"""
    rest = [c for c in T.CASES if c.form != "BREG8"]
    assert T.uncovered(rest) == ["no case takes (split, MUL, BREG8, 256x256)"]
    rest = [c for c in T.CASES if not (c.form == "HALO" and c.tile == (256, 256) and c.mode == 3)]
    assert T.uncovered(rest) == ["no case takes (split, MUL_UP2, HALO, 256x256)"]
    rest = [c for c in T.CASES if not (c.split and c.form == "PLAIN" and c.tile == (128, 64) and not c.switches and c.mode == 1)]
    assert T.uncovered(rest) == ["no case takes (split, FWD, PLAIN, 128x64) under default switches"]
    rest = [c for c in T.CASES if not (c.form in ("HALO", "BREG") and c.W == 17)]
    assert T.uncovered(rest) == ["no HALO case has: ragged columns", "no BREG case has: ragged columns"]
    rest = [c for c in T.CASES if not (not c.split and c.taps == 1 and c.form == "SMALL")]
    assert T.uncovered(rest) == ["no case takes (fp32, FWD, SMALL, 64x64) with one tap"]


def test_op_plan_asks_as_the_operator_launches():
    """the fragment-major weight copy exists for split backward 3x3 launches whose padded N is 64 or whose N % 256 == 0, and
    N / Cin are swapped for the backward modes"""
    MUL, BF = K.LRP_EPI_MUL, K.LRP_OPND_BF16X3
    c = T.Case(2, 28, 28, 64, 64, 9, 2, True, {}, "BREG", (128, 64), "")
    assert T.op_plan(c) == conv_plan(MUL, BF, 2, 28, 28, 64, 64, flags=K.LRP_PLAN_FRAG)
    assert T.op_plan(c)["form"] == K.LRP_FORM_BREG and conv_plan(MUL, BF, 2, 28, 28, 64, 64)["form"] != K.LRP_FORM_BREG
    c = T.Case(3, 14, 14, 40, 56, 9, 3, True, {}, "BREG", (128, 64), "")             # N = 40 pads to 64; S has 56 channels
    assert T.op_plan(c) == conv_plan(K.LRP_EPI_MUL_UP2, BF, 3, 14, 14, 40, 56, flags=K.LRP_PLAN_FRAG)
    c = T.Case(33, 56, 56, 256, 8, 9, 2, True, {}, "BREG8", (256, 256), "")
    assert T.op_plan(c) == conv_plan(MUL, BF, 33, 56, 56, 256, 8, flags=K.LRP_PLAN_FRAG)
    for c in (T.Case(2, 7, 5, 136, 72, 9, 2, True, {}, "", (), ""), T.Case(2, 28, 28, 64, 64, 9, 1, True, {}, "", (), ""),
              T.Case(2, 28, 28, 64, 64, 9, 2, False, {}, "", (), ""), T.Case(1, 1, 300, 64, 64, 1, 2, True, {}, "", (), "")):
        inC, N = T.launch_dims(c)
        assert T.op_plan(c) == conv_plan(T.EPI_OF_MODE[c.mode], BF if c.split else K.LRP_OPND_FP32, c.NB, c.H, c.W, N, inC, taps=c.taps)
    assert [T.conv_npad(n) for n in (8, 32, 33, 40, 64, 65, 72, 128, 136, 256)] == [32, 32, 64, 64, 64, 128, 128, 128, 256, 256]
