"""The launch plans of the rule table's mixed launches (csrc/conv_plan.h through lrp_conv_plan): every case of
tests/conv_rule_cases.py gets the form and tile it states, both kinds reach the staged, small and resident-image forms in both
operand formats, and what the plan refuses.  Pure host arithmetic: no GPU."""
import pytest

import conv_rule_cases as T
from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.engine import conv_plan, switches

MUL, UP2, FP, BF, DM = K.LRP_EPI_MUL, K.LRP_EPI_MUL_UP2, K.LRP_OPND_FP32, K.LRP_OPND_BF16X3, K.LRP_PLAN_DUAL_MUL


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_gets_its_plan(case):
    with switches(**case.switches):
        for pool in (False, True):
            p = T.op_plan(case, pool)
            assert p["ok"] == 1
            assert (T.FORM_NAMES[p["form"]], (p["BM"], p["BN"])) == (case.form, tuple(case.tile)), (T.plan_name(p), pool)
    if case.split:
        assert 9 * case.Cout >= T.MIN_SPLIT_K


def test_both_kinds_reach_every_family_of_forms():
    for kind in ("2to1", "1to2"):
        for split, forms in ((False, {"PLAIN", "SMALL"}), (True, {"PLAIN", "SMALL", "HALO"})):
            got = {c.form for c in T.CASES if c.kind == kind and c.split == split}
            assert got == forms, (kind, split, got)


def test_what_the_plan_refuses_of_a_mixed_launch():
    # one chain into two gates: the chain in whole pairs of groups, as the dual gate takes Cin
    assert conv_plan(MUL, BF, 3, 14, 14, 128, 72, flags=DM)["ok"] == 0
    assert conv_plan(MUL, BF, 3, 14, 14, 128, 80, flags=DM)["ok"] == 1
    assert conv_plan(UP2, FP, 3, 14, 14, 128, 12, flags=DM)["ok"] == 0
    assert conv_plan(UP2, FP, 3, 14, 14, 128, 16, flags=DM)["ok"] == 1
    # ... never on a weights-in-registers form or the 8-wave tile, whatever the chain count
    assert conv_plan(MUL, BF, 320, 28, 28, 512, 512, flags=DM | K.LRP_PLAN_FRAG)["ok"] == 0
    p = conv_plan(MUL, BF, 320, 28, 28, 512, 512, flags=DM)
    assert (p["form"], p["BM"], p["BN"]) == (K.LRP_FORM_HALO, 128, 128)
    # two chains into one gate is the single-gate launch over 2 Cout: split8 groups of 8, fp32 groups of 4
    assert conv_plan(MUL, BF, 3, 14, 14, 128, 2 * 12)["ok"] == 1 and conv_plan(MUL, BF, 3, 14, 14, 128, 2 * 10)["ok"] == 0
    assert conv_plan(MUL, FP, 3, 14, 14, 128, 2 * 6)["ok"] == 1
