"""The launch plan of the implicit-GEMM convolution (csrc/conv_plan.h conv_plan, through lrp_conv_plan, ABI v8): which form and
tile a launch takes, and which launches may carry the compact pool interface, the folded image layer or the fused pool.
Host arithmetic only — no GPU.  The launcher executes this plan and Encoder::explain / Encoder::encode ask the same function,
so what is asserted here is what runs."""
import itertools

import pytest

from lrp_imagecaptioning_amd import _capi as K
from lrp_imagecaptioning_amd.build import build_library
from lrp_imagecaptioning_amd.engine import conv_plan, switches
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG

PLAIN, SMALL, HALO, BREG, POOL = K.LRP_FORM_PLAIN, K.LRP_FORM_SMALL, K.LRP_FORM_HALO, K.LRP_FORM_BREG, K.LRP_FORM_POOL
UP2, IMG, POOLGC = K.LRP_PLAN_UP2_SRC, K.LRP_PLAN_IMG_PART, K.LRP_PLAN_POOL_GC


@pytest.fixture(scope="module", autouse=True)
def _library():
    build_library()


def _vgg16():
    """(name, cin, cout, H) per conv of VGG16 at 224 x 224"""
    H, out = 224, []
    for name, cin, cout, pool in VGG16_CFG:
        out.append((name, cin, cout, H))
        H = H // 2 if pool else H
    return out


def _walk(tokens, name, flags=0):
    """the dense split-bf16 reverse launch through a VGG16 layer: N = cin columns from cout channels; the layers with N <= 64
    have a fragment-major copy of their weights"""
    _, cin, cout, h = next(l for l in _vgg16() if l[0] == name)
    return conv_plan(K.LRP_EPI_MUL, K.LRP_OPND_BF16X3, tokens, h, h, cin, cout, flags=flags | (K.LRP_PLAN_FRAG if cin <= 64 else 0))


def _key(p):
    return (p["form"], p["BM"], p["BN"], p["tw"], p["th"], p["hrows"])


# tokens -> layer -> (form, BM, BN, tw, th, hrows)
_N64 = (BREG, 128, 64, 14, 9, 12)
_H128 = (HALO, 128, 128, 14, 9, 12)
_H256 = (HALO, 256, 256, 14, 18, 21)
_S64 = (SMALL, 64, 64, 0, 0, 0)
_MID = (PLAIN, 128, 64, 0, 0, 0)
WALK = {
    72: dict(block1_conv2=_N64, block2_conv1=_N64, block2_conv2=_H128, block3_conv1=_H128, block3_conv2=_H256, block3_conv3=_H256,
             block4_conv1=_H128, block4_conv2=_H256, block4_conv3=_H256, block5_conv1=_H128, block5_conv2=_H128, block5_conv3=_H128),
    3: dict(block1_conv2=_N64, block2_conv1=_N64, block2_conv2=_H128, block3_conv1=_S64, block3_conv2=_MID, block3_conv3=_MID,
            block4_conv1=_S64, block4_conv2=_S64, block4_conv3=_S64, block5_conv1=_S64, block5_conv2=_S64, block5_conv3=_S64),
    # (320 tokens of 14 rows: an 18-row tile crosses two image boundaries — 22 resident rows)
    320: dict(block1_conv2=_N64, block2_conv1=_N64, block2_conv2=_H128, block3_conv1=_H128, block3_conv2=_H256, block3_conv3=_H256,
              block4_conv1=_H256, block4_conv2=_H256, block4_conv3=_H256, block5_conv1=(HALO, 256, 256, 14, 18, 22),
              block5_conv2=(HALO, 256, 256, 14, 18, 22), block5_conv3=(HALO, 256, 256, 14, 18, 22)),
}


@pytest.mark.parametrize("tokens", sorted(WALK))
def test_vgg16_reverse_walk_forms(tokens):
    with switches(LRP_SPARSE_POOL=0):                      # (the plan is about the dense launches; the switch is not one of its inputs)
        for name, want in WALK[tokens].items():
            p = _walk(tokens, name)
            assert p["ok"] == 1 and _key(p) == want, (tokens, name, p)
            assert p["threads"] == (512 if p["BM"] == 256 else 256)


def test_vgg16_requests():
    # the folded image layer and the compact pool interface on block1_conv2: weights in registers, per-token tiles
    p = _walk(72, "block1_conv2", IMG | UP2)
    assert p["ok"] == 1 and p["form"] == BREG and (p["tw"], p["th"]) == (14, 9), p
    assert p["tpt"] == -(-224 // p["th"]) and p["hrows"] == p["th"] + 2 and p["m_tiles"] == 72 * p["tpt"] * 16, p
    assert _walk(72, "block1_conv2", UP2)["ok"] == 0       # (that kernel reads the compact interface with per-token tiles only)
    # the pipelined halo kernels take the compact interface; a grid of small tiles does not
    p = _walk(72, "block2_conv2", UP2)
    assert p["ok"] == 1 and _key(p) == _H128, p
    p = _walk(72, "block3_conv3", UP2)
    assert p["ok"] == 1 and _key(p) == _H256, p
    assert _walk(72, "block2_conv2", IMG)["ok"] == 0
    for name in ("block5_conv1", "block5_conv3", "block4_conv3", "block3_conv1"):
        assert _walk(3, name, UP2)["ok"] == 0, name
    with switches(LRP_UP2_PW=0):
        assert _walk(72, "block2_conv2", UP2)["ok"] == 0
        assert _walk(72, "block1_conv2", IMG | UP2)["ok"] == 1
    with switches(LRP_CONV_BREG=0):
        assert _walk(72, "block1_conv2", IMG)["ok"] == 0 and _walk(72, "block1_conv2", IMG | UP2)["ok"] == 0


def test_channel_counts():
    """split operands come in groups of 8 channels (fp32: any count), and the compact pool interface into the weights-in-registers
    kernel needs the whole A operand resident: at most 64 channels"""
    BF, F16, FP, MUL = K.LRP_OPND_BF16X3, K.LRP_OPND_F16X2, K.LRP_OPND_FP32, K.LRP_EPI_MUL
    for cin in (3, 12, 20, 68):
        assert conv_plan(MUL, BF, 8, 28, 28, 128, cin)["ok"] == 0
        assert conv_plan(MUL, F16, 8, 28, 28, 128, cin)["ok"] == 0
        assert conv_plan(K.LRP_EPI_IMG_STENCIL, BF, 8, 28, 28, 54, cin, taps=1)["ok"] == 0
        assert conv_plan(MUL, FP, 8, 28, 28, 128, cin)["ok"] == 1
    flags = K.LRP_PLAN_FRAG | IMG | UP2
    for cin, ok in ((8, 1), (56, 1), (64, 1), (72, 0), (128, 0)):
        p = conv_plan(MUL, BF, 72, 224, 224, 64, cin, flags=flags)
        assert p["ok"] == ok and (not ok or p["form"] == BREG), (cin, p)
        assert conv_plan(MUL, BF, 72, 224, 224, 64, cin, flags=K.LRP_PLAN_FRAG | IMG)["form"] == BREG   # (the fold alone does not care)


def test_vgg16_fused_pool():
    """the interleaved fp16-pair dual forward (N = 2 cout columns) with the pool in its epilogue"""
    def fwd(images, layer):
        _, cin, cout, h = layer
        return conv_plan(K.LRP_EPI_FWD_DUAL, K.LRP_OPND_F16X2, images, h, h, 2 * cout, cin, split=cout,
                         flags=K.LRP_PLAN_DUAL_IL | POOLGC)
    layers = _vgg16()
    pooled = [l for l, c in zip(layers, VGG16_CFG) if c[3]]
    assert [l[0] for l in pooled] == ["block1_conv2", "block2_conv2", "block3_conv3", "block4_conv3"]
    for images in (8, 32):
        for l in pooled:
            p = fwd(images, l)
            assert p["ok"] == 1 and _key(p) == (POOL, 128, 128, 14, 8, 11), (images, l[0], p)    # fill 0.875 >= 0.8
    for l in layers:
        if l[1] % 8 == 0:
            assert fwd(1, l)["ok"] == (1 if l[0] == "block1_conv2" else 0), l[0]
        if l[0].startswith("block5"):
            assert fwd(8, l)["ok"] == 0, l[0]
    with switches(LRP_POOL_FUSED=0):
        assert all(fwd(8, l)["ok"] == 0 for l in pooled)


SIZES = (1, 2, 5, 7, 14, 15, 28, 30)
WIDTHS = (8, 24, 64, 72, 128, 256, 512)
SETTINGS = [{}] + [{"LRP_CONV_HALO": v} for v in (0, 2)] + [{k: 0} for k in ("LRP_CONV_SMALL", "LRP_CONV_MID", "LRP_CONV_BREG",
                                                                           "LRP_UP2_PW", "LRP_POOL_FUSED")]


def _ceil(a, b):
    return -(-a // b)


def _check(p, NB, H, W, N, flags):
    assert 1 <= p["BM"] and 1 <= p["BN"] and p["threads"] in (256, 512)
    M = NB * H * W
    if p["form"] in (PLAIN, SMALL):
        assert flags & (UP2 | IMG | POOLGC) == 0, p        # a request is only ever carried by a resident-image form
        assert (p["tw"], p["th"], p["hrows"], p["tpt"]) == (0, 0, 0, 0)
        assert p["m_tiles"] == _ceil(M, p["BM"]) and p["n_tiles"] == _ceil(N, p["BN"]), p
        return
    assert p["form"] in (HALO, BREG, POOL), p
    tw, th, hrows = p["tw"], p["th"], p["hrows"]
    assert 1 <= tw <= 14 and th >= 1 and tw * th <= p["BM"], p
    assert hrows <= (22 if p["BM"] == 256 else 12), p
    assert p["n_tiles"] == _ceil(N, p["BN"]), p
    if p["tpt"]:                                           # per-token tiles: none straddles two tokens, no separator row inside
        assert flags & IMG and p["form"] == BREG
        assert p["tpt"] == _ceil(H, th) and hrows == th + 2 and p["m_tiles"] == NB * p["tpt"] * _ceil(W, tw), p
    else:
        assert not flags & IMG
        assert hrows == th + 2 + (th - 1 + H - 1) // H, p   # one separator row per image boundary a tile can cross
        assert p["m_tiles"] == _ceil(NB * H, th) * _ceil(W, tw), p
    if p["form"] == POOL:
        assert flags & POOLGC and tw % 2 == 0 and th % 2 == 0 and (p["BM"], p["BN"]) == (128, 128), p
    if p["form"] == BREG:
        assert (p["BM"], p["BN"], p["n_tiles"]) == (128, 64, 1), p
    if flags & UP2 and p["form"] == HALO:                  # the window loader of the pipelined kernels: two items per thread
        assert hrows * ((tw + 2) // 2 + 1) * 4 <= 2 * p["threads"], p


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "default" if not s else "%s=%s" % next(iter(s.items())))
def test_plan_properties(setting):
    MUL, DUAL, RELU = K.LRP_EPI_MUL, K.LRP_EPI_FWD_DUAL, K.LRP_EPI_BIAS_RELU
    BF, F16, FP = K.LRP_OPND_BF16X3, K.LRP_OPND_F16X2, K.LRP_OPND_FP32
    n = 0
    with switches(**setting):
        for H, W, N, NB, taps, Cin in itertools.product(SIZES, SIZES, WIDTHS, (1, 3, 5, 72), (9, 1), (64, 136)):
            frag = K.LRP_PLAN_FRAG if N <= 64 else 0
            asks = [(MUL, BF, 0, frag), (RELU, FP, 0, 0), (MUL, FP, 0, 0)]
            if taps == 9:
                asks += [(MUL, BF, 0, f | frag) for f in (UP2, IMG, IMG | UP2)]
            if N % 64 == 0:
                asks += [(DUAL, F16, N // 2, K.LRP_PLAN_DUAL_IL | f) for f in ((0, POOLGC) if taps == 9 else (0,))]
            for epi, prec, split, flags in asks:
                p = conv_plan(epi, prec, NB, H, W, N, Cin, taps=taps, split=split, flags=flags)
                n += 1
                if flags & (UP2 | IMG | POOLGC) == 0:
                    assert p["ok"] == 1, (H, W, N, NB, taps, epi, prec, p)
                if p["ok"]:
                    _check(p, NB, H, W, N, flags)
                    if p["form"] == BREG and flags & UP2:   # its window loader holds the whole A operand: two 32-channel chunks
                        assert Cin <= 64, p
                if setting.get("LRP_CONV_HALO") == 0:
                    assert p["form"] in (PLAIN, SMALL) and (p["ok"] == 1) == (flags & (UP2 | IMG | POOLGC) == 0)
                if setting.get("LRP_CONV_SMALL") == 0:
                    assert p["form"] != SMALL
    assert n > 10000
