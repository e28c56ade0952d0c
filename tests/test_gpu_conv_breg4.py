"""-m gpu: the 4-wave 128 x 128 resident-image tile with its weights in registers (csrc/conv_igemm.h FORM_BREG4 / FORM_BREG4_POOL)
against the pipelined kernel it replaces (LRP_CONV_BREG4=0).  Both issue, per output element, the same chain of MFMAs — chunk-major,
taps innermost, two k16 steps, al*bh, ah*bl, ah*bh (fp16 pairs: the TERMS rule per column tile; blocked accumulation flushed behind
the same taps) — so every comparison here is torch.equal.

Operator level (lrp_op_conv, mode 2 | LRP_CONV_SPLIT_BF16 | LRP_CONV_WREG: the entry packs the fragment-major copy) under
LRP_CONV_SMALL=0, LRP_CONV_MID=0, so that a handful of maps reach the 128-row tile.

Engine level: a VGG-like net at 56 x 56, widths 3 -> 64, 64 -> 64 pool, 64 -> 128, 128 -> 128 pool, 128 -> 320, 320 -> 320:
at 24 images x 7 words the walk has a compact producer (N = 128 from 320 channels at 14 x 14: ten chunks) and a compact consumer
(N = 128 at 28 x 28, the window loader) on the form, and the forward of the first two blocks runs on it, the pooled launches
included.  At this batch the 320-channel forward launches are small enough for the 128 x 64 tiles, so the forward with more than
eight chunks — a chunk with two flushes of the blocked accumulation (chunk & 7 == 7) and chunks with one — is run on the form in
a test of its own, under LRP_CONV_MID=0.  The library has no entry that reads a gate; the gates are compared through what reads
them: the heat-maps (LRP walk) and a gradient walk, which uses every gate — pooled and un-pooled — as a mask.
keep_acts (the fine-tune step's encode, lrp_train_begin) is reachable at this size and is run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l1
from gpu_util import report
from lrp_imagecaptioning_amd import _capi as K

pytestmark = pytest.mark.gpu
HALO, POOL, BREG4, BREG4_POOL = K.LRP_FORM_HALO, K.LRP_FORM_POOL, K.LRP_FORM_BREG4, K.LRP_FORM_BREG4_POOL
MUL, DUAL, BF, H2 = K.LRP_EPI_MUL, K.LRP_EPI_FWD_DUAL, K.LRP_OPND_BF16X3, K.LRP_OPND_F16X2
FRAG, UP2, IL, GC = K.LRP_PLAN_FRAG, K.LRP_PLAN_UP2_SRC, K.LRP_PLAN_DUAL_IL, K.LRP_PLAN_POOL_GC
GEOM = ("BM", "BN", "tw", "th", "hrows", "m_tiles", "n_tiles")

# NB, H, W, N (output columns: Cin of the layer), C (channels of S: Cout of the layer), LRP_CONV_HALO
CASES = [
    (3, 14, 14, 128, 40, 1),       # tiles span images, ragged second chunk
    (3, 14, 14, 128, 72, 1),       # the A buffers change hands twice
    (3, 14, 14, 256, 40, 1),       # two column tiles
    (2, 7, 5, 128, 72, 2),         # W < 14, H odd
    (2, 9, 17, 128, 40, 2),        # ragged last column tile
    (2, 28, 10, 128, 296, 2),      # ten chunks: the ring of weight registers wraps many times (tw = 10 fills 70 % of a tile: HALO=2)
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
    return conv_plan(MUL, BF, NB, H, W, N, C, flags=FRAG)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:5])))
def test_operator_is_bit_identical_to_the_pipelined_kernel(case):
    from lrp_imagecaptioning_amd.engine import op_conv, switches
    s, w, gate = _operands(case)
    outs, forms = {}, {}
    for on in (1, 0):
        with switches(LRP_CONV_BREG4=on, LRP_CONV_HALO=case[5], LRP_CONV_SMALL=0, LRP_CONV_MID=0):
            forms[on] = _plan(case)
            outs[on] = op_conv(s, w, None, gate, 2, 9, split_bf16=True, wreg=True).clone()
            if on:
                plain = op_conv(s, w, None, gate, 2, 9, split_bf16=True).clone()   # without the bit: the pipelined kernel, as before
    assert forms[1]["form"] == BREG4 and forms[0]["form"] == HALO and (forms[0]["BM"], forms[0]["BN"]) == (128, 128), forms
    assert all(forms[1][k] == forms[0][k] for k in GEOM), forms
    assert bool(torch.isfinite(outs[1]).all()) and float(outs[1].abs().sum()) > 0
    assert torch.equal(outs[1], outs[0]), float((outs[1] - outs[0]).abs().max())
    assert torch.equal(plain, outs[0])
    report("conv_breg4_%s" % "x".join(map(str, case[:5])), bit_identical=True, form=forms[1]["form"])


def test_operator_against_fp32():
    """the bound tests/test_gpu_conv_breg8.py holds the split path to, against the exact-fp32 operator (mode 2 without the flags)"""
    from lrp_imagecaptioning_amd.engine import op_conv, switches
    case = CASES[1]
    s, w, gate = _operands(case)
    with switches(LRP_CONV_SMALL=0, LRP_CONV_MID=0):
        assert _plan(case)["form"] == BREG4
        got = op_conv(s, w, None, gate, 2, 9, split_bf16=True, wreg=True).cpu().numpy()
    ref = op_conv(s, w, None, gate, 2, 9).cpu().numpy()
    err = rel_l1(got, ref)
    report("conv_breg4_vs_fp32", case=list(case[:5]), rel_l1=err)
    assert err < 2e-5, err
    st = s.double().cpu().permute(0, 3, 1, 2)
    wt = torch.as_tensor(w, dtype=torch.float64).permute(3, 2, 0, 1)
    c64 = F.conv_transpose2d(st, wt, padding=1).permute(0, 2, 3, 1).numpy() * gate.double().cpu().numpy()
    assert rel_l1(got, c64) < 2e-5


def test_the_mode_bit_is_refused_where_it_does_not_apply():
    from lrp_imagecaptioning_amd.engine import op_conv
    s, w, gate = _operands((2, 6, 6, 64, 40))
    with pytest.raises(Exception):
        op_conv(s, w, None, gate, 2, 9, split_bf16=True, wreg=True)           # Cin % 128 != 0
    s, w, gate = _operands((2, 6, 6, 128, 40))
    with pytest.raises(Exception):
        op_conv(s, w, None, gate, 2, 9, wreg=True)                            # not the split path


# ---- engine level
CFG = [("b1c1", 3, 64, False), ("b1c2", 64, 64, True), ("b2c1", 64, 128, False), ("b2c2", 128, 128, True),
       ("b3c1", 128, 320, False), ("b3c2", 320, 320, False)]
HW, L, D, HID, V = 56, 196, 320, 64, 60


@pytest.fixture(scope="module")
def net():
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, vgg_weights
    rs = np.random.RandomState(7)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, D, HID, HID, V))
    made = {}

    def engine(B, T, precision="bf16x3"):
        key = (B, T, precision)
        if key not in made:
            e = LRPEngine(decoder="adaptive", cnn_cfg=CFG, img_hw=(HW, HW), L=L, D=D, H=HID, E=HID, V=V, max_images=B,
                          max_tokens=B * T, max_caption_len=T + 1)
            if precision != "bf16x3":
                e.set_precision(precision)
            e.set_weights(w)
            made[key] = e
        return made[key]
    return engine


def _inputs(B, T):
    from lrp_imagecaptioning_amd.synthetic import captions
    rs = np.random.RandomState(B)
    X = torch.as_tensor(rs.uniform(-120, 130, size=(B, HW, HW, 3)).astype(np.float32)).cuda()
    return X, captions(rs, B, T, V), torch.as_tensor(rs.standard_normal((2, L, D)).astype(np.float32)).cuda()


def _explain(eng, X, caps, T, head=None):
    """heat-maps, features and (head given) a gradient walk of the first two images: every gate as a mask"""
    B = X.shape[0]
    eng.encode_images(X)
    feat = eng.get_features().clone()
    eng.decoder_forward(caps)
    hm = eng.explain_tokens([b for b in range(B) for _ in range(T)], [t for _ in range(B) for t in range(1, T + 1)])[0].clone()
    assert bool(torch.isfinite(hm).all()) and float(hm.abs().sum()) > 0
    out = [hm, feat]
    if head is not None:
        out.append(eng.cnn_walk([0, min(1, B - 1)], head, "gradient").clone())
    return out


def _plans(B, T, terms):
    """the launches of this net that the form is for: walk (producer, consumer with the window loader), forward of blocks 1 and 2"""
    from lrp_imagecaptioning_amd.engine import conv_plan
    walk = [conv_plan(MUL, BF, B * T, 14, 14, 128, 320, flags=FRAG), conv_plan(MUL, BF, B * T, 28, 28, 128, 128, flags=FRAG | UP2)]
    fwd = [conv_plan(DUAL, H2, B, 56, 56, 128, 64, terms=terms[1], split=64, flags=FRAG | IL | GC),
           conv_plan(DUAL, H2, B, 28, 28, 256, 64, terms=terms[2], split=128, flags=FRAG | IL),
           conv_plan(DUAL, H2, B, 28, 28, 256, 128, terms=terms[3], split=128, flags=FRAG | IL | GC)]
    return walk, fwd


@pytest.mark.parametrize("precision", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("B,T,reaches", [(24, 7, True), (2, 3, False)], ids=["168tokens", "6tokens"])
def test_engine_is_bit_identical_with_the_switch_off_and_on_a_single_image_handle(net, B, T, reaches, precision):
    from lrp_imagecaptioning_amd.engine import switches
    X, caps, head = _inputs(B, T)
    # (f16x2: the forward's Z+ column tiles are two-term below the last pool — TERMS 23 — and the walk is not on the form)
    terms = {1: 23, 2: 23, 3: 23} if precision == "f16x2" else {1: 7, 2: 7, 3: 7}
    walk, fwd = _plans(B, T, terms)
    if reaches:
        assert [p["form"] for p in fwd] == [BREG4_POOL, BREG4, BREG4_POOL], fwd
        assert precision != "bf16x3" or [p["form"] for p in walk] == [BREG4, BREG4], walk
    else:
        assert all(p["form"] not in (BREG4, BREG4_POOL) for p in walk + fwd), (walk, fwd)
    big = net(B, T, precision)
    on = _explain(big, X, caps, T, head)
    with switches(LRP_CONV_BREG4=0):
        off_walk, off_fwd = _plans(B, T, terms)
        assert all(p["form"] not in (BREG4, BREG4_POOL) for p in off_walk + off_fwd)
        off = _explain(big, X, caps, T, head)
    for a, b, what in zip(on, off, ("heat-maps", "features", "gradient walk")):
        assert torch.equal(a, b), (what, float((a - b).abs().max()))
    one = net(1, T, precision)
    i = B // 2
    alone = _explain(one, X[i:i + 1], caps[i:i + 1], T)
    assert torch.equal(on[1][i:i + 1], alone[1])                               # the forward: the part of f16x2 that is on the form
    if precision == "bf16x3":                                                  # (f16x2 heat-maps: the test below)
        assert torch.equal(on[0][i * T:(i + 1) * T], alone[0])
    report("breg4_engine_%s_%d_tokens" % (precision, B * T), bit_identical=True, forms=[p["form"] for p in walk + fwd])


def test_f16x2_heatmaps_of_one_image_on_a_single_image_handle(net):
    """The fp16-pair mode end to end: 24 images x 7 words against the same image on a B = 1 handle.  The B = 1 forward runs on
    64 x 64 tiles (one column tile per wave), the batch on the form: both must give the Z+ blocks of the interleaved matrix their
    two-term product (TERMS bit 4, by the block's place in the matrix) — before that rule the two differed by 4.0e-7 (relative
    L1 3.0e-6) [MI355X]."""
    B, T = 24, 7
    X, caps, _ = _inputs(B, T)
    on = _explain(net(B, T, "f16x2"), X, caps, T)
    i = B // 2
    alone = _explain(net(1, T, "f16x2"), X[i:i + 1], caps[i:i + 1], T)
    d = (on[0][i * T:(i + 1) * T] - alone[0]).abs()
    report("breg4_f16x2_single_image", max_abs=float(d.max()), rel_l1=float(d.sum() / alone[0].abs().sum()))
    assert torch.equal(on[0][i * T:(i + 1) * T], alone[0]), (float(d.max()), float(d.sum() / alone[0].abs().sum()))


def test_forward_of_ten_chunks_flushes_where_the_pipelined_loop_does(net):
    """320 -> 320 at 14 x 14: ten channel chunks, kc = 9 chunk + tap, flushed behind every kc with kc & 7 == 7 — chunk 7 flushes
    twice (taps 0 and 8), the others once.  LRP_CONV_MID=0 keeps the 24-image launch on the 128 x 128 tile."""
    from lrp_imagecaptioning_amd.engine import conv_plan, switches
    B, T = 24, 7
    X, caps, head = _inputs(B, T)
    big = net(B, T)
    feats = {}
    for on in (1, 0):
        with switches(LRP_CONV_BREG4=on, LRP_CONV_MID=0):
            p = conv_plan(DUAL, H2, B, 14, 14, 640, 320, split=320, flags=FRAG | IL)
            assert p["form"] == (BREG4 if on else HALO) and (p["BM"], p["BN"]) == (128, 128), p
            big.encode_images(X)
            feats[on] = big.get_features().clone()
    assert bool(torch.isfinite(feats[1]).all()) and float(feats[1].abs().sum()) > 0
    assert torch.equal(feats[1], feats[0]), float((feats[1] - feats[0]).abs().max())


def test_keep_acts_encode_is_bit_identical(net):
    """the fine-tune step's encode (lrp_train_begin: activations kept, pools as passes of their own) on the form and off it"""
    from lrp_imagecaptioning_amd.engine import LRPEngine, switches
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, vgg_weights
    B, T = 24, 7
    X, caps, _ = _inputs(B, T)
    rs = np.random.RandomState(7)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    w.update(adaptive_weights(rs, L, D, HID, HID, V))
    e = LRPEngine(decoder="adaptive", cnn_cfg=CFG, img_hw=(HW, HW), L=L, D=D, H=HID, E=HID, V=V, max_images=B, max_tokens=B * T,
                  max_caption_len=T + 1)
    e.set_weights(w)
    e.train_begin()
    on = _explain(e, X, caps, T)
    with switches(LRP_CONV_BREG4=0):
        off = _explain(e, X, caps, T)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
