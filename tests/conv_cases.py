"""The operator cases of the implicit-GEMM convolution (lrp_op_conv), each with the launch plan it must get: one table for
tests/test_conv_op_coverage.py (CPU: every case gets the plan it states, and the table reaches every kernel form the operator can
take) and tests/test_gpu_conv_forms.py (GPU: every case against a float64 convolution).  A plain helper module like gpu_util.py.

A case is (NB, H, W, Cin, Cout, taps, mode, split) as lrp_op_conv takes them — mode 0 bias + relu, 1 bias, 2 gate multiply of the
transposed conv, 3 the same through a 2x2 pool; the backward modes map Cout channels of S to Cin output columns — plus the
switches it runs under and the form and tile conv_plan (csrc/conv_plan.h) must answer under them."""
from collections import namedtuple

from lrp_imagecaptioning_amd import _capi as K

Case = namedtuple("Case", "NB H W Cin Cout taps mode split switches form tile note")

FORM_NAMES = {K.LRP_FORM_PLAIN: "PLAIN", K.LRP_FORM_SMALL: "SMALL", K.LRP_FORM_HALO: "HALO", K.LRP_FORM_BREG: "BREG",
              K.LRP_FORM_POOL: "POOL", K.LRP_FORM_IMG: "IMG", K.LRP_FORM_BREG8: "BREG8"}
EPI_OF_MODE = (K.LRP_EPI_BIAS_RELU, K.LRP_EPI_BIAS, K.LRP_EPI_MUL, K.LRP_EPI_MUL_UP2)
EPI_NAMES = ("BIAS_RELU", "BIAS", "MUL", "MUL_UP2")
RESIDENT = ("HALO", "BREG", "BREG8")

# switch sets.  LARGE takes the small-grid rules out of the way, so that a stack of two or three images reaches the large tiles
DEFAULT = {}
LARGE = {"LRP_CONV_SMALL": 0, "LRP_CONV_MID": 0}
HALO0, HALO1, HALO2 = (dict(LARGE, LRP_CONV_HALO=v) for v in (0, 1, 2))
NO_BREG = dict(LARGE, LRP_CONV_BREG=0)
NO_BREG8 = {"LRP_CONV_BREG8": 0}


# The element bar of the split-bf16 operator (gpu_util.elem_bar) charges the three-term product 2^-16.  That is the dropped lo*lo'
# term alone; the two lo halves are themselves rounded (2^-17 each), so the arithmetic's own worst case is 2^-15 per product, which
# a sum of K products approaches only for tiny K: the IDEAL split of Gaussian operands, evaluated in float64, scores 1.8e-5 at
# K = 8 over 26 M outputs (above the bar), 5e-6 at K = 72, 0.6e-6 ... 3.6e-6 up to K = 4608 (tests/test_elem_metric.py).  The bar is
# derived for K >= 72 — the shallowest real layer, 3 x 3 x 8 — and every split case keeps its K = taps x input channels there.
MIN_SPLIT_K = 72


def _cases(shape, taps, split, switches, form, tile, modes, note=""):
    return [Case(*shape, taps, m, split, switches, form, tile, note) for m in modes]


CASES = (
    # ---------------- fp32 operands: staged tiles only
    _cases((2, 7, 5, 136, 72), 9, False, LARGE, "PLAIN", (128, 128), (0, 1, 2, 3), "ragged M (70 rows), two N tiles backward")
    + _cases((3, 14, 14, 128, 128), 9, False, LARGE, "PLAIN", (128, 64), (0, 1, 2, 3), "the halved tile of a grid under 2200 blocks")
    + _cases((2, 6, 6, 16, 24), 9, False, DEFAULT, "PLAIN", (128, 32), (0, 1, 2, 3), "N <= 32, Cin < 32")
    + _cases((2, 7, 5, 136, 72), 9, False, DEFAULT, "SMALL", (64, 64), (0, 1, 2, 3), "ragged M and N on 64 x 64 tiles")
    + _cases((1, 1, 300, 64, 136), 1, False, LARGE, "PLAIN", (128, 128), (1,), "one tap, two N tiles, ragged M")
    + _cases((1, 1, 300, 64, 96), 1, False, DEFAULT, "SMALL", (64, 64), (1, 2), "one tap")
    # ---------------- split-bf16 operands, staged tiles
    + _cases((3, 14, 14, 128, 128), 9, True, HALO0, "PLAIN", (128, 128), (1, 2, 3), "ragged M (588 rows)")
    + _cases((2, 28, 28, 64, 64), 9, True, NO_BREG, "PLAIN", (128, 64), (1, 2, 3), "N = 64 without the weights in registers")
    + _cases((2, 6, 6, 16, 24), 9, True, DEFAULT, "PLAIN", (128, 32), (1, 2, 3), "N <= 32")
    + _cases((33, 56, 56, 8, 256), 9, True, {"LRP_CONV_HALO": 0}, "PLAIN", (256, 256), (1,), "8-wave tile, >= 400 blocks")
    + _cases((33, 56, 56, 72, 256), 1, True, DEFAULT, "PLAIN", (256, 256), (1,), "8-wave tile, one tap (K = 72: see MIN_SPLIT_K)")
    + _cases((2, 7, 5, 136, 72), 9, True, DEFAULT, "SMALL", (64, 64), (1, 2, 3), "ragged M and N on 64 x 64 tiles")
    + _cases((3, 28, 28, 8, 1024), 9, True, DEFAULT, "PLAIN", (128, 64), (1,), "in-between rule: 19 x 8 large tiles -> 128 x 64")
    + _cases((3, 28, 28, 1024, 8), 9, True, DEFAULT, "PLAIN", (128, 64), (2, 3), "in-between rule: 19 x 8 large tiles -> 128 x 64")
    # ---------------- split-bf16 operands, resident image, 128-row tiles
    + _cases((3, 14, 14, 128, 128), 9, True, HALO1, "HALO", (128, 128), (1, 2, 3), "tw 14 th 9: tiles span images")
    + _cases((1, 9, 33, 128, 136), 9, True, HALO2, "HALO", (128, 128), (1, 2, 3), "tw 11: three column tiles, H odd, two N tiles forward")
    + _cases((2, 7, 5, 136, 72), 9, True, HALO2, "HALO", (128, 128), (1, 2, 3),
             "tw 5 th 8: W < 14, H odd, tiles span images, Cin % 32 != 0, two N tiles backward")
    + _cases((2, 16, 16, 128, 128), 9, True, HALO2, "HALO", (128, 128), (1, 2, 3), "tw 8: power-of-two width")
    + _cases((2, 9, 17, 128, 136), 9, True, HALO2, "HALO", (128, 128), (1, 2, 3), "tw 9 on W 17: ragged last column tile, H odd")
    + _cases((2, 28, 28, 64, 64), 9, True, HALO2, "HALO", (128, 64), (1,), "tw 14 th 9: two column tiles")
    + _cases((2, 7, 5, 56, 40), 9, True, HALO2, "HALO", (128, 64), (1,), "tw 5 th 8: W < 14, H odd, Cin % 32 != 0")
    + _cases((2, 28, 28, 64, 64), 9, True, DEFAULT, "BREG", (128, 64), (2, 3), "two chunks: one group of the resident image")
    + _cases((3, 14, 14, 40, 56), 9, True, DEFAULT, "BREG", (128, 64), (2, 3), "tiles span images, N = 40 < 64, Cin % 32 != 0")
    + _cases((2, 7, 5, 56, 40), 9, True, HALO2, "BREG", (128, 64), (2, 3), "tw 5 th 8: W < 14, H odd, tiles span images")
    + _cases((2, 9, 17, 64, 40), 9, True, HALO2, "BREG", (128, 64), (2, 3), "tw 9 on W 17: ragged last column tile, H odd")
    # ---------------- split-bf16 operands, resident image, 8-wave 256 x 256 tiles (>= 400 blocks: about 100 k rows)
    + _cases((33, 56, 56, 8, 256), 9, True, DEFAULT, "HALO", (256, 256), (1,), "tw 14 th 18: tiles span images")
    + _cases((33, 56, 56, 256, 8), 9, True, NO_BREG8, "HALO", (256, 256), (2,), "the pipelined kernel behind FORM_BREG8")
    + _cases((33, 56, 56, 256, 8), 9, True, DEFAULT, "HALO", (256, 256), (3,), "the pooled epilogue on the 8-wave tile")
    + _cases((33, 56, 56, 256, 8), 9, True, DEFAULT, "BREG8", (256, 256), (2,), "weights in registers on the 8-wave tile")
)


def case_id(c):
    sw = ",".join("%s=%s" % (k[4:] if k.startswith("LRP_") else k, v) for k, v in sorted(c.switches.items())) or "default"
    return "%s-%s-%dx%d-%s-%s-%dtap-%s" % ("split" if c.split else "fp32", c.form, c.tile[0], c.tile[1], EPI_NAMES[c.mode],
                                            "x".join(map(str, c[:5])), c.taps, sw)


def conv_npad(n):
    """csrc/conv_plan.h conv_npad: the output columns padded to the tile width their count picks"""
    bn = 128 if n > 64 else 64 if n > 32 else 32
    return -(-n // bn) * bn


def launch_dims(c):
    """(channels of the input tensor, output columns N) of the launch: swapped for the backward modes"""
    return (c.Cout, c.Cin) if c.mode >= 2 else (c.Cin, c.Cout)


def op_plan(c):
    """conv_plan asked exactly as lrp_op_conv launches the case, under the switches in force at the call: the epilogue of the
    mode, N and Cin swapped for the backward modes, and LRP_PLAN_FRAG where the entry packs a fragment-major weight copy —
    split, backward, 9 taps, and the padded N is 64 or N % 256 == 0."""
    from lrp_imagecaptioning_amd.engine import conv_plan
    inC, N = launch_dims(c)
    frag = bool(c.split) and c.mode >= 2 and c.taps == 9 and (conv_npad(N) == 64 or N % 256 == 0)
    return conv_plan(EPI_OF_MODE[c.mode], K.LRP_OPND_BF16X3 if c.split else K.LRP_OPND_FP32, c.NB, c.H, c.W, N, inC, taps=c.taps,
                     flags=K.LRP_PLAN_FRAG if frag else 0)


def plan_name(p):
    """'HALO 128x128 tw14 th9' / 'PLAIN 128x64' of a conv_plan answer"""
    s = "%s %dx%d" % (FORM_NAMES[p["form"]], p["BM"], p["BN"])
    return s + (" tw%d th%d" % (p["tw"], p["th"]) if p["tw"] else "")


def geometry(c, p):
    """What a resident-image plan `p` of case `c` exercises, as a set of names."""
    if FORM_NAMES[p["form"]] not in RESIDENT:
        return set()
    inC, _ = launch_dims(c)
    th, rows = p["th"], c.NB * c.H
    spans = any(y0 // c.H != min(y0 + th - 1, rows - 1) // c.H for y0 in range(0, rows, th))
    feats = {"spans images": spans, "ragged columns": c.W % p["tw"] != 0, "W < 14": c.W < 14, "H odd": c.H % 2 == 1,
             "n_tiles > 1": p["n_tiles"] > 1, "Cin % 32 != 0": inC % 32 != 0}
    return {k for k, v in feats.items() if v}


# ---- what the table must reach: every (operand format, epilogue, form, tile) that lrp_op_conv can take.  "FWD" is BIAS or
# BIAS_RELU.  `default` = under default switches (the in-between rule only exists there).
Need = namedtuple("Need", "fmt epi form tile taps default")


def _needs():
    out = []
    for form, tile in (("PLAIN", (128, 128)), ("PLAIN", (128, 64)), ("PLAIN", (128, 32)), ("SMALL", (64, 64))):
        out += [Need("fp32", e, form, tile, 9, False) for e in ("FWD", "MUL", "MUL_UP2")]
    out += [Need("fp32", "FWD", "PLAIN", (128, 128), 1, False), Need("fp32", "FWD", "SMALL", (64, 64), 1, False)]
    for tile in ((128, 128), (128, 64), (128, 32)):
        out += [Need("split", e, "PLAIN", tile, 9, False) for e in ("FWD", "MUL", "MUL_UP2")]
    out += [Need("split", "FWD", "PLAIN", (256, 256), 9, False), Need("split", "FWD", "PLAIN", (256, 256), 1, False)]
    out += [Need("split", e, "SMALL", (64, 64), 9, False) for e in ("FWD", "MUL", "MUL_UP2")]
    out += [Need("split", e, "PLAIN", (128, 64), 9, True) for e in ("FWD", "MUL", "MUL_UP2")]      # the in-between rule
    out += [Need("split", e, "HALO", (128, 128), 9, False) for e in ("FWD", "MUL", "MUL_UP2")]
    out += [Need("split", "FWD", "HALO", (128, 64), 9, False)]
    out += [Need("split", e, "HALO", (256, 256), 9, False) for e in ("FWD", "MUL", "MUL_UP2")]
    out += [Need("split", e, "BREG", (128, 64), 9, False) for e in ("MUL", "MUL_UP2")]
    out += [Need("split", "MUL", "BREG8", (256, 256), 9, False)]
    return out


NEEDS = _needs()
GEOMETRY_NEEDS = {"HALO": ("spans images", "ragged columns", "W < 14", "H odd", "n_tiles > 1", "Cin % 32 != 0"),
                  "BREG": ("spans images", "ragged columns", "W < 14", "H odd", "Cin % 32 != 0")}      # (BREG: one N tile by construction)


def meets(c, need):
    epi = "FWD" if c.mode < 2 else EPI_NAMES[c.mode]
    return (("split" if c.split else "fp32"), epi, c.form, tuple(c.tile), c.taps) == need[:5] and (not need.default or not c.switches)


def uncovered(cases):
    """-> list of messages, one per Need and per geometry feature that no case of `cases` reaches: the stated plans are
    trusted here (test_conv_op_coverage checks them against conv_plan first)."""
    from lrp_imagecaptioning_amd.engine import switches
    miss = ["no case takes (%s, %s, %s, %dx%d)%s%s" % (n.fmt, n.epi, n.form, n.tile[0], n.tile[1], " with one tap" if n.taps == 1 else "",
                                                       " under default switches" if n.default else "")
            for n in NEEDS if not any(meets(c, n) for c in cases)]
    seen = {f: set() for f in GEOMETRY_NEEDS}
    for c in cases:
        if c.form in seen:
            with switches(**c.switches):
                seen[c.form] |= geometry(c, op_plan(c))
    miss += ["no %s case has: %s" % (f, g) for f, want in GEOMETRY_NEEDS.items() for g in want if g not in seen[f]]
    return miss
