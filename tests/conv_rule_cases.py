"""The operator cases of the rule table's two mixed launches (lrp_op_conv_rule), each with the launch plan it must get: one table
for tests/test_conv_plan_rule.py (CPU) and tests/test_gpu_rule_table.py (GPU: every case, with and without the pool, against a
float64 evaluation).  The idea of tests/conv_ab_cases.py.

A case is (kind, NB, H, W, Cin, Cout, split): "2to1" reads two chains of Cout channels and applies one gate — the plain MUL
epilogues over Cin(plan) = 2 Cout; "1to2" reads one chain and applies two gates — LRP_PLAN_DUAL_MUL over Cin(plan) = Cout, which
the plan takes in multiples of 16 (split) / 8 (fp32).  Every split case keeps 9 x Cout >= conv_cases.MIN_SPLIT_K per chain."""
from collections import namedtuple

from conv_cases import DEFAULT, FORM_NAMES, HALO0, HALO1, HALO2, LARGE, MIN_SPLIT_K, plan_name  # noqa: F401
from lrp_imagecaptioning_amd import _capi as K

Case = namedtuple("Case", "kind NB H W Cin Cout split switches form tile note")

CASES = (
    # ---------------- two chains in, one gate out
    Case("2to1", 2, 7, 5, 136, 72, False, LARGE, "PLAIN", (128, 128), "ragged M (70 rows), two N tiles, K = 144 channels per tap"),
    Case("2to1", 2, 6, 6, 16, 24, False, DEFAULT, "PLAIN", (128, 32), "N <= 32, one and a half chunks per tap"),
    Case("2to1", 2, 7, 5, 136, 72, False, DEFAULT, "SMALL", (64, 64), "ragged M and N on 64 x 64 tiles"),
    Case("2to1", 3, 14, 14, 128, 128, True, HALO0, "PLAIN", (128, 128), "ragged M (588 rows), tiles spanning images"),
    Case("2to1", 2, 6, 6, 16, 24, True, DEFAULT, "PLAIN", (128, 32), "N <= 32"),
    Case("2to1", 2, 7, 5, 136, 72, True, DEFAULT, "SMALL", (64, 64), "ragged M and N on 64 x 64 tiles"),
    Case("2to1", 2, 7, 5, 136, 72, True, HALO2, "HALO", (128, 128), "tw 5 th 8: W < 14, H odd, 2 Cout % 32 != 0, two N tiles"),
    Case("2to1", 2, 28, 28, 64, 64, True, HALO2, "HALO", (128, 64), "the single gate takes the resident image at N = 64"),
    # ---------------- one chain in, two gates out
    Case("1to2", 2, 7, 5, 136, 72, False, LARGE, "PLAIN", (128, 128), "ragged M, two N tiles"),
    Case("1to2", 3, 14, 14, 128, 128, False, LARGE, "PLAIN", (128, 64), "the halved tile of a grid under 2200 blocks"),
    Case("1to2", 2, 6, 6, 16, 24, False, DEFAULT, "PLAIN", (128, 32), "N <= 32, K = 24 channels per tap: under one chunk"),
    Case("1to2", 2, 7, 5, 136, 72, False, DEFAULT, "SMALL", (64, 64), "ragged M and N on 64 x 64 tiles"),
    Case("1to2", 3, 14, 14, 128, 128, True, HALO0, "PLAIN", (128, 128), "ragged M (588 rows)"),
    Case("1to2", 2, 28, 28, 64, 64, True, HALO2, "PLAIN", (128, 64), "N = 64: the dual gate stays staged"),
    Case("1to2", 2, 6, 6, 16, 16, True, DEFAULT, "PLAIN", (128, 32), "N <= 32, the narrowest chain the plan takes (16)"),
    Case("1to2", 3, 14, 14, 128, 128, True, DEFAULT, "SMALL", (64, 64), "64 x 64 tiles"),
    Case("1to2", 3, 14, 14, 128, 128, True, HALO1, "HALO", (128, 128), "tw 14 th 9: tiles span images"),
    Case("1to2", 2, 16, 16, 128, 128, True, HALO2, "HALO", (128, 128), "tw 8: power-of-two width"),
)


def case_id(c):
    sw = ",".join("%s=%s" % (k[4:] if k.startswith("LRP_") else k, v) for k, v in sorted(c.switches.items())) or "default"
    return "%s-%s-%s-%dx%d-%s-%s" % (c.kind, "split" if c.split else "fp32", c.form, c.tile[0], c.tile[1], "x".join(map(str, c[1:6])), sw)


def chains_gates(c):
    return (2, 1) if c.kind == "2to1" else (1, 2)


def op_plan(c, pool):
    """conv_plan asked exactly as lrp_op_conv_rule launches the case under the switches in force at the call"""
    from lrp_imagecaptioning_amd.engine import conv_plan
    ch, g = chains_gates(c)
    return conv_plan(K.LRP_EPI_MUL_UP2 if pool else K.LRP_EPI_MUL, K.LRP_OPND_BF16X3 if c.split else K.LRP_OPND_FP32, c.NB, c.H, c.W,
                     c.Cin, ch * c.Cout, flags=K.LRP_PLAN_DUAL_MUL if g == 2 else 0)
