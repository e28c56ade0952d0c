"""-m gpu: the 8-wave 256 x 256 resident-image tile with its weights in registers (csrc/conv_igemm.h FORM_BREG8) against the
pipelined kernel it replaces (LRP_CONV_BREG8=0).  Both issue, per output element, the same chain of MFMAs — chunk-major, taps
innermost, two k16 steps, al*bh, ah*bl, ah*bh — so every comparison here is torch.equal.

Operator level (lrp_op_conv, mode 2 | LRP_CONV_SPLIT_BF16; the entry packs the fragment-major copy, so the plan is asked with
LRP_PLAN_FRAG): the smallest stacks that still reach the form — a grid of >= 400 tiles of 256 x 256, i.e. 72 maps of 28 x 28 at
N = 512, 264 of 14 x 14, 184 of 10 x 28 / 28 x 10, and for N = 256 (one column tile) 132 maps of 28 x 28.  (120 maps of
28 x 28 at N = 256 are 368 tiles: that launch keeps the 128 x 128 tile under either setting; it is run as well.)
28 x 10 fills a 256-row tile to 74 % only (tw = 10, th = 19), which the plan takes under LRP_CONV_HALO=2.

Engine level: a 3-block VGG-like net at 56 x 56, widths 64 / 256 / 512.  72 tokens (no launch of that size reaches 400 tiles)
and 264 tokens (the top conv's launch does), switch on against off, and one image on a B = 1 handle against the same image
inside the batch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l1
from gpu_util import report
from lrp_imagecaptioning_amd import _capi as K

pytestmark = pytest.mark.gpu
HALO, BREG8 = K.LRP_FORM_HALO, K.LRP_FORM_BREG8

# NB, H, W, N (output columns: Cin of the layer), C (channels of S: Cout of the layer), LRP_CONV_HALO, reaches the form
CASES = [
    (72, 28, 28, 512, 40, 1, True),      # two chunks, the second ragged (8 of 32 channels)
    (72, 28, 28, 512, 72, 1, True),      # two chunks and a ragged third: the A buffers change hands twice
    (264, 14, 14, 512, 40, 1, True),     # an 18-row tile crosses two map boundaries: 22 resident rows, separator rows
    (184, 10, 28, 512, 40, 1, True),     # H != W, 18-row tiles over 10-row maps, ragged last row band
    (184, 28, 10, 512, 40, 2, True),     # H != W, tw = 10: 190 of a tile's 256 rows are pixels
    (132, 28, 28, 256, 40, 1, True),     # one column tile
    (120, 28, 28, 256, 40, 1, False),    # 368 tiles: below the grid rule, 128 x 128 tiles either way
]


def _operands(case):
    NB, H, W, N, C = case[:5]
    rs = np.random.RandomState(sum(case[:5]))
    s = torch.as_tensor(rs.standard_normal((NB, H, W, C)).astype(np.float32)).cuda()
    w = np.abs(rs.standard_normal((3, 3, N, C)) / np.sqrt(9 * N)).astype(np.float32)
    gate = torch.as_tensor(rs.uniform(0, 1, size=(NB, H, W, N)).astype(np.float32)).cuda()
    return s, w, gate


def _plan(case):
    from lrp_imagecaptioning_amd.engine import conv_plan
    NB, H, W, N, C = case[:5]
    return conv_plan(K.LRP_EPI_MUL, K.LRP_OPND_BF16X3, NB, H, W, N, C, flags=K.LRP_PLAN_FRAG)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])))
def test_operator_is_bit_identical_to_the_pipelined_kernel(case):
    from lrp_imagecaptioning_amd.engine import op_conv, switches
    s, w, gate = _operands(case)
    outs, forms = {}, {}
    for on in (1, 0):
        with switches(LRP_CONV_BREG8=on, LRP_CONV_HALO=case[5]):
            forms[on] = _plan(case)
            outs[on] = op_conv(s, w, None, gate, 2, 9, split_bf16=True).clone()
    if case[6]:
        assert forms[1]["form"] == BREG8 and forms[0]["form"] == HALO and forms[0]["BM"] == 256, forms
        assert all(forms[1][k] == forms[0][k] for k in ("tw", "th", "hrows", "m_tiles", "n_tiles")), forms
    else:
        assert forms[1] == forms[0] and forms[1]["form"] != BREG8, forms
    assert bool(torch.isfinite(outs[1]).all()) and float(outs[1].abs().sum()) > 0
    assert torch.equal(outs[1], outs[0]), float((outs[1] - outs[0]).abs().max())
    report("conv_breg8_%s" % "x".join(map(str, case[:5])), bit_identical=True, form=forms[1]["form"])


def test_operator_against_fp32():
    """the bound tests/test_gpu_conv_op.py holds the split path to, against the exact-fp32 operator (mode 2 without the flag)"""
    from lrp_imagecaptioning_amd.engine import op_conv
    case = CASES[1]
    s, w, gate = _operands(case)
    assert _plan(case)["form"] == BREG8
    got = op_conv(s, w, None, gate, 2, 9, split_bf16=True).cpu().numpy()
    ref = op_conv(s, w, None, gate, 2, 9).cpu().numpy()
    err = rel_l1(got, ref)
    report("conv_breg8_vs_fp32", case=list(case[:5]), rel_l1=err)
    assert err < 2e-5, err
    # and the fp32 operator itself against the float64 convolution, on a few maps
    st = s[:4].double().cpu().permute(0, 3, 1, 2)
    wt = torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1)
    c64 = F.conv_transpose2d(st, wt, padding=1).permute(0, 2, 3, 1).numpy() * gate[:4].double().cpu().numpy()
    assert rel_l1(got[:4], c64) < 2e-5


# ---- engine level
CFG = [("b1c1", 3, 64, False), ("b1c2", 64, 64, True), ("b2c1", 64, 256, False), ("b2c2", 256, 256, True),
       ("b3c1", 256, 512, False), ("b3c2", 512, 512, False)]
HW, L, D, HID, V = 56, 196, 512, 64, 60


@pytest.fixture(scope="module")
def net():
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, vgg_weights
    rs = np.random.RandomState(5)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, D, HID, HID, V))

    def engine(B, T):
        e = LRPEngine(decoder="adaptive", cnn_cfg=CFG, img_hw=(HW, HW), L=L, D=D, H=HID, E=HID, V=V, max_images=B,
                      max_tokens=B * T, max_caption_len=T + 1)
        e.set_weights(w)
        return e
    return engine


def _explain(eng, X, caps, T):
    B = X.shape[0]
    eng.encode_images(X)
    eng.decoder_forward(caps)
    hm = eng.explain_tokens([b for b in range(B) for _ in range(T)], [t for _ in range(B) for t in range(1, T + 1)])[0].clone()
    assert bool(torch.isfinite(hm).all()) and float(hm.abs().sum()) > 0
    return hm


@pytest.mark.parametrize("B,T,reaches", [(8, 9, False), (24, 11, True)], ids=["72tokens", "264tokens"])
def test_heatmaps_are_bit_identical_with_the_switch_off_and_on_a_single_image_handle(net, B, T, reaches):
    from lrp_imagecaptioning_amd.engine import conv_plan, switches
    from lrp_imagecaptioning_amd.synthetic import captions
    rs = np.random.RandomState(B)
    X = torch.as_tensor(rs.uniform(-120, 130, size=(B, HW, HW, 3)).astype(np.float32)).cuda()
    caps = captions(rs, B, T, V)
    # the launch through the top conv: N = 512 columns from 512 channels at 14 x 14
    top = conv_plan(K.LRP_EPI_MUL, K.LRP_OPND_BF16X3, B * T, 14, 14, 512, 512, flags=K.LRP_PLAN_FRAG)
    assert (top["form"] == BREG8) == reaches, top
    big = net(B, T)
    on = _explain(big, X, caps, T)
    with switches(LRP_CONV_BREG8=0):
        off = _explain(big, X, caps, T)
    assert torch.equal(on, off), float((on - off).abs().max())
    assert torch.equal(_explain(big, X, caps, T), on)
    one = net(1, T)
    i = B // 2
    alone = _explain(one, X[i:i + 1], caps[i:i + 1], T)
    assert torch.equal(on[i * T:(i + 1) * T], alone)
    report("breg8_engine_%d_tokens" % (B * T), bit_identical=True, top_form=top["form"])
