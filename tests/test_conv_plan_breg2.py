"""LRP_CONV_BREG2 chooses between the two loops of the 128 x 64 weights-in-registers kernel (csrc/conv_igemm.h, FORM_BREG) in the
launcher, not in the plan: over the sweep of tests/test_conv_plan.py::test_plan_properties every field of lrp_conv_plan's answer
is the same with the switch off and on.  Host arithmetic only — no GPU."""
import itertools

import pytest

from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.build import build_library
from lrp_imagecaptioning_amd.engine import PLAN_FIELDS, conv_plan, switches

UP2, IMG, POOLGC = K.LRP_PLAN_UP2_SRC, K.LRP_PLAN_IMG_PART, K.LRP_PLAN_POOL_GC
SIZES = (1, 2, 5, 7, 14, 15, 28, 30)
WIDTHS = (8, 24, 64, 72, 128, 256, 512)


@pytest.fixture(scope="module", autouse=True)
def _library():
    build_library()


def _sweep():
    MUL, DUAL, RELU = K.LRP_EPI_MUL, K.LRP_EPI_FWD_DUAL, K.LRP_EPI_BIAS_RELU
    BF, F16, FP = K.LRP_OPND_BF16X3, K.LRP_OPND_F16X2, K.LRP_OPND_FP32
    out = []
    for H, W, N, NB, taps, Cin in itertools.product(SIZES, SIZES, WIDTHS, (1, 3, 5, 72), (9, 1), (64, 136)):
        frag = K.LRP_PLAN_FRAG if N <= 64 else 0
        asks = [(MUL, BF, 0, frag), (RELU, FP, 0, 0), (MUL, FP, 0, 0)]
        if taps == 9:
            asks += [(MUL, BF, 0, f | frag) for f in (UP2, IMG, IMG | UP2)]
        if N % 64 == 0:
            asks += [(DUAL, F16, N // 2, K.LRP_PLAN_DUAL_IL | f) for f in ((0, POOLGC) if taps == 9 else (0,))]
        for epi, prec, split, flags in asks:
            p = conv_plan(epi, prec, NB, H, W, N, Cin, taps=taps, split=split, flags=flags)
            out.append(tuple(p[k] for k in PLAN_FIELDS))
    return out


def test_every_answer_is_the_same_with_the_switch_off_and_on():
    with switches(LRP_CONV_BREG2=1):
        on = _sweep()
    with switches(LRP_CONV_BREG2=0):
        off = _sweep()
    default = _sweep()
    assert len(on) > 10000
    assert on == off and on == default
    assert any(p[0] == 1 and p[1] == K.LRP_FORM_BREG for p in on)          # the sweep does reach the form


def test_the_vgg16_launches_keep_their_plan():
    """block2_conv1 and block1_conv2 (dense, and folded with the compact pool interface) at 320 tokens"""
    BF, MUL, FRAG = K.LRP_OPND_BF16X3, K.LRP_EPI_MUL, K.LRP_PLAN_FRAG
    for sw_ in (0, 1):
        with switches(LRP_CONV_BREG2=sw_):
            p = conv_plan(MUL, BF, 320, 112, 112, 64, 128, flags=FRAG)
            assert (p["ok"], p["form"], p["BM"], p["BN"], p["tw"], p["th"], p["hrows"], p["n_tiles"], p["threads"]) == \
                   (1, K.LRP_FORM_BREG, 128, 64, 14, 9, 12, 1, 256), p
            q = conv_plan(MUL, BF, 320, 224, 224, 64, 64, flags=FRAG | IMG | UP2)
            assert q["ok"] == 1 and q["form"] == K.LRP_FORM_BREG and q["tpt"] == 25 and q["hrows"] == 11 and \
                   q["m_tiles"] == 320 * 25 * 16, q
