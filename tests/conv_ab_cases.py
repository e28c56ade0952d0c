"""The operator cases of the two-chain launch of the alpha-beta walk (lrp_op_conv_ab), each with the launch plan it must get:
one table for tests/test_conv_plan_ab.py (CPU: every case gets the plan it states, and the table reaches every form conv_plan
can answer for LRP_PLAN_DUAL_MUL) and tests/test_gpu_alphabeta.py (GPU: every case, with and without the pool, against a float64
evaluation).  The idea of tests/conv_cases.py, for the other operator.

A case is (NB, H, W, Cin, Cout, split) as lrp_op_conv_ab takes them: S+ and S- have Cout channels each, the launch reduces over
K = 9 x 2 Cout and writes Cin columns per chain.  Every split case keeps 9 x Cout >= conv_cases.MIN_SPLIT_K per chain."""
from collections import namedtuple

from conv_cases import DEFAULT, FORM_NAMES, HALO0, HALO1, HALO2, LARGE, MIN_SPLIT_K, plan_name  # noqa: F401
from lrp_imagecaptioning_amd import _capi as K

Case = namedtuple("Case", "NB H W Cin Cout split switches form tile note")

CASES = (
    # ---------------- fp32 operands: staged tiles only
    Case(2, 7, 5, 136, 72, False, LARGE, "PLAIN", (128, 128), "ragged M (70 rows), two N tiles"),
    Case(3, 14, 14, 128, 128, False, LARGE, "PLAIN", (128, 64), "the halved tile of a grid under 2200 blocks"),
    Case(2, 6, 6, 16, 24, False, DEFAULT, "PLAIN", (128, 32), "N <= 32, K = 48 channels per tap: one and a half chunks"),
    Case(2, 7, 5, 136, 72, False, DEFAULT, "SMALL", (64, 64), "ragged M and N on 64 x 64 tiles"),
    # ---------------- split-bf16 operands, staged tiles
    Case(3, 14, 14, 128, 128, True, HALO0, "PLAIN", (128, 128), "ragged M (588 rows), tiles spanning images"),
    Case(2, 28, 28, 64, 64, True, LARGE, "PLAIN", (128, 64), "N = 64 (never the weights-in-registers form)"),
    Case(2, 28, 28, 64, 64, True, HALO2, "PLAIN", (128, 64), "N = 64 stays staged under LRP_CONV_HALO=2 as well"),
    Case(2, 6, 6, 16, 24, True, DEFAULT, "PLAIN", (128, 32), "N <= 32"),
    Case(2, 7, 5, 136, 72, True, DEFAULT, "SMALL", (64, 64), "ragged M and N on 64 x 64 tiles"),
    Case(3, 28, 28, 1024, 8, True, DEFAULT, "PLAIN", (128, 64), "in-between rule: 19 x 8 large tiles -> 128 x 64"),
    # ---------------- split-bf16 operands, resident image (pipelined 128 x 128 tile)
    Case(3, 14, 14, 128, 128, True, HALO1, "HALO", (128, 128), "tw 14 th 9: tiles span images"),
    Case(2, 16, 16, 128, 128, True, HALO2, "HALO", (128, 128), "tw 8: power-of-two width"),
    Case(2, 7, 5, 136, 72, True, HALO2, "HALO", (128, 128), "tw 5 th 8: W < 14, H odd, tiles span images, 2 Cout % 32 != 0, two N tiles"),
)

# every (operand format, form, tile) conv_plan can answer for LRP_PLAN_DUAL_MUL; each case runs both epilogues (pool or not)
NEEDS = ([("fp32", f, t) for f, t in (("PLAIN", (128, 128)), ("PLAIN", (128, 64)), ("PLAIN", (128, 32)), ("SMALL", (64, 64)))]
         + [("split", f, t) for f, t in (("PLAIN", (128, 128)), ("PLAIN", (128, 64)), ("PLAIN", (128, 32)), ("SMALL", (64, 64)),
                                         ("HALO", (128, 128)))])


def case_id(c):
    sw = ",".join("%s=%s" % (k[4:] if k.startswith("LRP_") else k, v) for k, v in sorted(c.switches.items())) or "default"
    return "%s-%s-%dx%d-%s-%s" % ("split" if c.split else "fp32", c.form, c.tile[0], c.tile[1], "x".join(map(str, c[:5])), sw)


def op_plan(c, pool):
    """conv_plan asked exactly as lrp_op_conv_ab launches the case under the switches in force at the call"""
    from lrp_imagecaptioning_amd.engine import conv_plan
    return conv_plan(K.LRP_EPI_MUL_UP2 if pool else K.LRP_EPI_MUL, K.LRP_OPND_BF16X3 if c.split else K.LRP_OPND_FP32, c.NB, c.H, c.W,
                     c.Cin, 2 * c.Cout, flags=K.LRP_PLAN_DUAL_MUL)


def uncovered(cases):
    return ["no case takes (%s, %s, %dx%d)" % (fmt, form, tile[0], tile[1]) for fmt, form, tile in NEEDS
            if not any((("split" if c.split else "fp32"), c.form, tuple(c.tile)) == (fmt, form, tile) for c in cases)]
