"""The launch plan's FORM_BREG8 (csrc/conv_plan.h conv_plan, through lrp_conv_plan): the dense split-bf16 EPI_MUL launches of the
reverse walk that take the 8-wave 256 x 256 tile run it with the weights in registers when a fragment-major copy of the weights
exists.  Host arithmetic only — no GPU."""
import pytest

from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.build import build_library
from lrp_imagecaptioning_amd.engine import conv_plan, switches
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG

HALO, BREG8 = K.LRP_FORM_HALO, K.LRP_FORM_BREG8
MUL, BF = K.LRP_EPI_MUL, K.LRP_OPND_BF16X3
FRAG, UP2 = K.LRP_PLAN_FRAG, K.LRP_PLAN_UP2_SRC
GEOM = ("BM", "BN", "tw", "th", "hrows", "m_tiles", "n_tiles")
# the walk's dense launches on the 8-wave tile at the bench size (block3_conv3 / block4_conv3 run on the 2:4-sparse kernels)
LAYERS = ("block5_conv3", "block5_conv2", "block5_conv1", "block4_conv2", "block4_conv1", "block3_conv2")


@pytest.fixture(scope="module", autouse=True)
def _library():
    build_library()


def _walk(tokens, name, flags=0):
    H = 224
    for n, cin, cout, pool in VGG16_CFG:
        if n == name:
            return conv_plan(MUL, BF, tokens, H, H, cin, cout, flags=flags)
        H = H // 2 if pool else H
    raise KeyError(name)


def test_constant():
    assert K.LRP_FORM_BREG8 == 6


@pytest.mark.parametrize("name", LAYERS)
def test_vgg16_walk_takes_the_form_with_todays_geometry(name):
    today = _walk(320, name)
    assert today["ok"] == 1 and today["form"] == HALO and (today["BM"], today["BN"], today["threads"]) == (256, 256, 512), today
    p = _walk(320, name, FRAG)
    assert p["ok"] == 1 and p["form"] == BREG8 and p["threads"] == 512, p
    assert [p[k] for k in GEOM] == [today[k] for k in GEOM], (p, today)


@pytest.mark.parametrize("name", LAYERS)
def test_without_the_copy_with_a_request_or_switched_off_it_is_the_pipelined_kernel(name):
    today = _walk(320, name)
    up2 = _walk(320, name, UP2)
    assert _walk(320, name, FRAG | UP2) == up2 and (up2["ok"] == 0 or up2["form"] == HALO), up2
    with switches(LRP_CONV_BREG8=0):
        assert _walk(320, name, FRAG) == today
    assert _walk(320, name, FRAG)["form"] == BREG8                 # and back


def test_three_tokens_take_nothing_of_it():
    for name, cin, cout, pool in VGG16_CFG[1:]:
        assert _walk(3, name, FRAG)["form"] != BREG8, name


def test_other_launches_keep_their_forms():
    # fp32 / fp16-pair operands, the pooled epilogue, one tap, the residual tail, N % 256 != 0: never
    F = K.LRP_PLAN_FRAG
    assert conv_plan(MUL, K.LRP_OPND_FP32, 320, 28, 28, 512, 512, flags=F)["form"] != BREG8
    assert conv_plan(MUL, K.LRP_OPND_F16X2, 320, 28, 28, 512, 512, flags=F)["form"] != BREG8
    assert conv_plan(K.LRP_EPI_MUL_UP2, BF, 320, 28, 28, 512, 512, flags=F)["form"] != BREG8
    assert conv_plan(MUL, BF, 320, 28, 28, 512, 512, taps=1, flags=F)["form"] != BREG8
    assert conv_plan(MUL, BF, 320, 28, 28, 512, 512, flags=F | K.LRP_PLAN_JOIN)["form"] != BREG8
    assert conv_plan(MUL, BF, 320, 28, 28, 384, 512, flags=F)["form"] != BREG8
    assert conv_plan(MUL, BF, 320, 28, 28, 512, 512, flags=F)["form"] == BREG8
