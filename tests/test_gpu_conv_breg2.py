"""-m gpu: the chunk loop of the 4-wave 128 x 64 weights-in-registers tile (csrc/conv_igemm.h, FORM_BREG with the kernel's C2 axis:
the N <= 64 launches of the dense split-bf16 walk) against the tile's first loop (LRP_CONV_BREG2=0).  Both issue, per output
element, the same chain of MFMAs — chunk-major, taps innermost, two k16 steps, al*bh, ah*bl, ah*bh — so every comparison between
the two is torch.equal; the plan's answer is the same under both (tests/test_conv_plan_breg2.py).

Operator level (lrp_op_conv, mode 2 | LRP_CONV_SPLIT_BF16; the entry packs the fragment-major copy for N <= 64): S of 32 .. 160
channels = one chunk (no hand-over of the A buffers), two, three (odd: buffer parity, the clamped prefetch past the end), four and
five, on stacks of 3 maps at 5 x 14 (a tile crosses image boundaries: separator rows; LRP_CONV_HALO=2 as the 8-row tile fills
87.5 %), 10 x 15 (ragged last row band, column strips of 8 and 7 pixels: LRP_CONV_HALO=2, the fill is 53 %) and 28 x 28.  N = 64, N = 40 (padded columns of this
tile) and N = 8 (the narrow tile: not on the form, the switch must change nothing).

Engine level: conv 3 -> 64, conv 64 -> 64 + pool, conv 64 -> 64 — the walk's top launch is a dense compact producer on the form, the
launch below it the folded one (image layer in its epilogue, per-token tiles, the compact pool interface: the PW instantiation)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l1
from gpu_util import report
from lrp_imagecaptioning_amd import _capi as K

pytestmark = pytest.mark.gpu
BREG, MUL, BF = K.LRP_FORM_BREG, K.LRP_EPI_MUL, K.LRP_OPND_BF16X3
FRAG, UP2, IMG = K.LRP_PLAN_FRAG, K.LRP_PLAN_UP2_SRC, K.LRP_PLAN_IMG_PART

SHAPES = [(3, 5, 14, 2), (3, 10, 15, 2), (3, 28, 28, 1)]            # NB, H, W, LRP_CONV_HALO
CHANNELS = [32, 64, 96, 128, 160]


def _operands(NB, H, W, N, C):
    rs = np.random.RandomState(NB + H + W + N + C)
    s = torch.as_tensor(rs.standard_normal((NB, H, W, C)).astype(np.float32)).cuda()
    w = np.abs(rs.standard_normal((3, 3, N, C)) / np.sqrt(9 * N)).astype(np.float32)
    gate = torch.as_tensor(rs.uniform(0, 1, size=(NB, H, W, N)).astype(np.float32)).cuda()
    return s, w, gate


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_operator_is_bit_identical_to_the_first_loop(shape, C):
    from lrp_imagecaptioning_amd.engine import conv_plan, op_conv, switches
    NB, H, W, halo = shape
    for N in (64, 40, 8):
        s, w, gate = _operands(NB, H, W, N, C)
        outs, plans = {}, {}
        for on in (1, 0):
            with switches(LRP_CONV_BREG2=on, LRP_CONV_HALO=halo):
                plans[on] = conv_plan(MUL, BF, NB, H, W, N, C, flags=FRAG)
                outs[on] = op_conv(s, w, None, gate, 2, 9, split_bf16=True).clone()
        assert plans[1] == plans[0], plans
        assert (plans[1]["form"] == BREG) == (N > 32), plans
        if N > 32:
            assert (plans[1]["BM"], plans[1]["BN"], plans[1]["n_tiles"]) == (128, 64, 1), plans
        assert bool(torch.isfinite(outs[1]).all()) and float(outs[1].abs().sum()) > 0
        assert torch.equal(outs[1], outs[0]), (N, float((outs[1] - outs[0]).abs().max()))
        if N == 64:
            st = s.double().cpu().permute(0, 3, 1, 2)
            wt = torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1)
            c64 = F.conv_transpose2d(st, wt, padding=1).permute(0, 2, 3, 1).numpy() * gate.double().cpu().numpy()
            err = rel_l1(outs[1].cpu().numpy(), c64)
            report("conv_breg2_%dx%dx%d_C%d" % (NB, H, W, C), bit_identical=True, rel_l1_vs_float64=err)
            assert err < 2e-5, err


# ---- engine level
CFG = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 64, False)]
HID, V = 32, 40


def _engine(hw, B, T, w):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    L = (hw[0] // 2) * (hw[1] // 2)
    e = LRPEngine(decoder="adaptive", cnn_cfg=CFG, img_hw=hw, L=L, D=64, H=HID, E=HID, V=V, max_images=B, max_tokens=max(B * T, 4),
                  max_caption_len=T + 1)
    e.set_weights(w)
    return e


# (20 x 30: three column strips of 14 fill 71 % of the tiles, and a launch that carries a request is held to the default fill — the
#  plan refuses the fold there and the image layer runs as a launch of its own; 20 x 28 is the same height on the folded launch)
@pytest.mark.parametrize("hw,folded", [((18, 28), True), ((20, 30), False), ((20, 28), True)], ids=lambda s: "%dx%d" % s if isinstance(s, tuple) else "")
def test_folded_launch_is_bit_identical_and_batch_invariant(hw, folded):
    from oracle import cnn_lrp_ref as C
    from lrp_imagecaptioning_amd.engine import conv_plan, switches
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, captions, vgg_weights
    B, T = 2, 3
    L = (hw[0] // 2) * (hw[1] // 2)
    rs = np.random.RandomState(hw[0])
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, 64, HID, HID, V))
    Xn = rs.uniform(-120, 130, size=(B, hw[0], hw[1], 3)).astype(np.float32)
    X = torch.as_tensor(Xn).cuda()
    caps = captions(rs, B, T, V)
    idx, tpos = [0, 1, 1], [1, 2, 3]                       # 3 tokens of 2 images
    # the folded launch takes the compact pool interface; the producer above it is a dense launch on the form
    for on in (1, 0):
        with switches(LRP_CONV_BREG2=on):
            p = conv_plan(MUL, BF, len(idx), hw[0], hw[1], 64, 64, flags=FRAG | IMG | UP2)
            assert p["ok"] == (1 if folded else 0), p
            if folded:
                assert p["form"] == BREG and p["tpt"] == -(-hw[0] // p["th"]), p
                assert conv_plan(MUL, BF, len(idx), hw[0] // 2, hw[1] // 2, 64, 64, flags=FRAG)["form"] == BREG
    big = _engine(hw, B, T, w)
    Rn = np.abs(rs.standard_normal((len(idx), L, 64))).astype(np.float32)
    R = torch.as_tensor(Rn).cuda()

    def run(eng, Xs, cs, ii):
        eng.encode_images(Xs)
        eng.decoder_forward(cs)
        hm = eng.explain_tokens(ii, tpos[:len(ii)])[0].clone()
        return hm

    on = run(big, X, caps, idx)
    on_R = big.cnn_explain(idx, R).clone()
    with switches(LRP_CONV_BREG2=0):
        off = run(big, X, caps, idx)
        off_R = big.cnn_explain(idx, R).clone()
    assert bool(torch.isfinite(on).all()) and float(on.abs().sum()) > 0
    assert torch.equal(on, off), float((on - off).abs().max())
    assert torch.equal(on_R, off_R), float((on_R - off_R).abs().max())
    one = _engine(hw, 1, T, w)
    for i in range(B):
        rows = [j for j, b in enumerate(idx) if b == i]
        one.encode_images(X[i:i + 1])
        one.decoder_forward(caps[i:i + 1])
        alone = one.explain_tokens([0] * len(rows), [tpos[j] for j in rows])[0]
        assert torch.equal(alone, on[rows]), (i, float((alone - on[rows]).abs().max()))
    # the float64 evaluation of the walk
    layers = C.vgg_layers(w, CFG)
    ref = C.analyze(layers, Xn[idx], Rn.reshape(len(idx), hw[0] // 2, hw[1] // 2, 64))
    err = max(rel_l1(on_R[j].cpu().numpy(), ref[j]) for j in range(len(idx)))
    report("conv_breg2_folded_%dx%d" % hw, bit_identical=True, rel_l1_vs_float64=err)
    assert err < 1e-4, err


def test_vgg16_heatmaps_are_bit_identical_with_the_switch_off():
    """VGG16 at 224 x 224, 2 images x 2 words, default path: block2_conv1 (four chunks) and the folded block1_conv2 on the chunk loop"""
    from oracle import cnn_lrp_ref as C
    from lrp_imagecaptioning_amd.engine import LRPEngine, switches
    from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, adaptive_weights, captions, images, vgg_weights
    B, T, Vv = 2, 2, 200
    eng = LRPEngine(decoder="adaptive", V=Vv, max_images=B, max_tokens=B * T, max_caption_len=T + 1)
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    w.update(adaptive_weights(rs, 196, 512, 512, 512, Vv))
    eng.set_weights(w)
    Xn = images(rs, B)
    X = torch.as_tensor(Xn).cuda()
    caps = captions(rs, B, T, Vv)
    idx = [b for b in range(B) for _ in range(T)]
    tpos = [t for _ in range(B) for t in range(1, T + 1)]
    Rn = np.abs(rs.standard_normal((1, 196, 512))).astype(np.float32)
    R = torch.as_tensor(Rn).cuda()
    res = {}
    for on in (1, 0):
        with switches(LRP_CONV_BREG2=on):
            eng.encode_images(X)
            eng.decoder_forward(caps)
            res[on] = (eng.explain_tokens(idx, tpos)[0].clone(), eng.cnn_explain([1], R).clone())
    hm = res[1][0]
    assert bool(torch.isfinite(hm).all()) and all(float(hm[j].abs().sum()) > 0 for j in range(B * T))
    assert torch.equal(res[1][0], res[0][0]), float((res[1][0] - res[0][0]).abs().max())
    assert torch.equal(res[1][1], res[0][1])
    ref = C.analyze(C.vgg_layers(w, VGG16_CFG), np.asarray(Xn[1:2], dtype=np.float32), Rn.reshape(1, 14, 14, 512))
    err = rel_l1(res[1][1][0].cpu().numpy(), ref[0])
    report("conv_breg2_vgg16", bit_identical=True, rel_l1_vs_float64=err)
    assert err < 1e-4, err
