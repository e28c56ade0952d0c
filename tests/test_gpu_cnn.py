"""-m gpu: CNN half of the hot path (lrp_encode_images + lrp_cnn_explain ==
LRPSequentialPresetA.analyze([X,R]), E:179-181) against the float64 literal
oracle (oracle/cnn_lrp_ref.py).  Tolerance: BASELINE.json's 1e-4 relative L1."""
import numpy as np
import pytest
import torch

from conftest import rel_l1
from gpu_util import band_bar, band_rel_l1, report
from lrp_imagecaptioning_amd.synthetic import VGG16_CFG, images, vgg_weights
from oracle import cnn_lrp_ref as C

pytestmark = pytest.mark.gpu
TOL = 1e-4

TINY_CFG = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, False), ("c4", 16, 16, True), ("c5", 16, 16, False)]
MID_CFG = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, True), ("c4", 128, 256, False), ("c5", 256, 128, False)]


def _engine(cfg, hw, B, ntok, w):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    side = hw
    for _, _, _, p in cfg:
        side = side // 2 if p else side
    eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=(hw, hw), L=side * side, D=cfg[-1][2], H=32, E=32, V=50,
                    max_images=B, max_tokens=ntok, max_caption_len=4)
    eng.set_weights(w)
    return eng, side


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("name,cfg,hw,B", [("tiny", TINY_CFG, 16, 3), ("mid", MID_CFG, 32, 2)])
def test_small_nets_match_oracle(name, cfg, hw, B, prec):
    rs = np.random.RandomState(7)
    w = vgg_weights(rs, cfg, bias_std=0.3)
    layers = C.vgg_layers(w, cfg)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    eng, side = _engine(cfg, hw, B, 2 * B, w)
    eng.set_precision(prec)
    eng.encode_images(X)
    feat = eng.get_features().cpu().numpy().reshape(B, side, side, -1)
    feat_ref = C.forward(layers, X)
    assert rel_l1(feat, feat_ref) < 1e-5
    # two relevance maps per image, tokens interleaved to exercise the token -> image map
    idx = [b for b in range(B)] + [B - 1 - b for b in range(B)]
    R = (rs.standard_normal((2 * B,) + feat_ref.shape[1:]) * feat_ref[idx]).astype(np.float32)
    out = eng.cnn_explain(idx, R).cpu().numpy()
    ref = C.analyze(layers, X[idx], R)
    errs = [rel_l1(out[i], ref[i]) for i in range(2 * B)]
    # the worst single image row / column as well (gpu_util.band_rel_l1), held to 10 x the float32 oracle's own figure
    bar, band32 = band_bar(C.analyze(layers, X[idx], R, dtype=torch.float32), ref)
    band = max(band_rel_l1(out[i], ref[i], where=True) for i in range(2 * B))
    report("cnn_" + name + "_" + prec, max_rel_l1=max(errs), worst_band=band[0], worst_band_at=band[1],
           f32_restatement_band=band32, band_bar=bar)
    assert np.isfinite(out).all()
    assert band[0] < bar, (band, bar)
    # f16x2 (opt-in fast mode) reads one fp16 per weight only where a sum has >= 576 products (C_out >= 64): these narrow nets
    # keep the three-term product in every layer (two-term measured 6e-5 on the tiny net: nothing to average over)
    assert max(errs) < TOL, errs


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16x3_fast", "f16x2"])
def test_vgg16_full_size_matches_oracle(prec):
    """BASELINE geometry: 224x224, VGG16 to block5_conv3, 2 images x 2 relevance maps, in every arithmetic mode:
    exact fp32 MFMA / split-bf16 reverse walk (default) / split-bf16 forward activations too (opt-in; its heat-map
    error is dominated by the handful of max-pool arg-max flips a 1e-5 activation error causes)."""
    rs = np.random.RandomState(0)
    w = vgg_weights(rs)
    layers = C.vgg_layers(w, VGG16_CFG)
    X = images(rs, 2)
    eng, side = _engine(VGG16_CFG, 224, 2, 4, w)
    assert side == 14
    eng.set_precision(prec)
    eng.encode_images(X)
    feat = eng.get_features().cpu().numpy().reshape(2, 14, 14, 512)
    feat_ref = C.forward(layers, X)
    e_feat = rel_l1(feat, feat_ref)
    idx = [0, 1, 1, 0]
    R = (rs.standard_normal((4, 14, 14, 512)) * feat_ref[idx]).astype(np.float32)
    out = eng.cnn_explain(idx, R).cpu().numpy()
    ref = C.analyze(layers, X[idx], R)
    errs = [rel_l1(out[i], ref[i]) for i in range(4)]
    report("cnn_vgg16_" + prec, feat_rel_l1=e_feat, max_rel_l1=max(errs))
    assert e_feat < (1e-5 if prec != "bf16x3_fast" else 5e-5)
    # every mode holds the reference bar on these dense He-normal kernels (f16x2 measured 1.2e-6 here; on sparse heavy-tailed
    # kernels it does not: tests/test_gpu_stress_parity.py — which is why bf16x3 is the default)
    assert max(errs) < TOL, errs
    # linearity in R (size-independent property): analyze(a*R1 + R2) = a*analyze(R1) + analyze(R2)
    out2 = eng.cnn_explain([0, 0], np.stack([2.5 * R[0] + R[3], R[3]])).cpu().numpy()
    assert rel_l1(out2[0], 2.5 * out[0] + out[3]) < (1e-5 if prec == "fp32" else 5e-5)
    # (f16x2: the weight rounding is the same linear map for every R, so linearity holds far below its parity figure)


def test_state_errors():
    from lrp_imagecaptioning_amd.engine import LRPEngine
    rs = np.random.RandomState(1)
    w = vgg_weights(rs, TINY_CFG)
    eng, side = _engine(TINY_CFG, 16, 2, 2, w)
    with pytest.raises(RuntimeError):                    # explain before encode
        eng.cnn_explain([0], np.zeros((1, side * side, 16), np.float32))
    eng.encode_images(rs.uniform(-100, 100, size=(2, 16, 16, 3)).astype(np.float32))
    with pytest.raises(ValueError):                      # image index out of range
        eng.cnn_explain([5], np.zeros((1, side * side, 16), np.float32))
    with pytest.raises(ValueError):
        eng.set_weights({"c1_W": np.zeros((3, 3, 3, 9), np.float32)})
    with pytest.raises(NotImplementedError):
        LRPEngine(decoder="transformer")


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "f16x2"])
def test_maxpool_exact_ties_follow_first_in_scan_order(prec):
    """Known-answer case for the one semantics SURVEY 7 leaves 'believed equal': the routing of relevance through a
    2x2 max-pool (RA:470-480 -> IL:138-157, tf.gradients of MaxPooling2D) when a window holds EXACT positive ties or
    is all zero after the ReLU.  Small-integer images / weights / biases make every activation an exactly
    representable integer in float64 (oracle), fp32 and split-bf16 alike, so the ties are the same ties on both
    sides; the oracle routes to the first maximum in window scan order (torch max_pool2d == the rule the
    restatement documents), the HIP path must agree element for element."""
    cfg = [("c1", 3, 8, True), ("c2", 8, 8, True), ("c3", 8, 16, False)]
    hw, Bn = 16, 2
    rs = np.random.RandomState(42)
    w = {}
    for name, cin, cout, _ in cfg:
        w[name + "_W"] = rs.randint(-1, 2, size=(3, 3, cin, cout)).astype(np.float32)
        w[name + "_b"] = rs.randint(-2, 3, size=(cout,)).astype(np.float32)
    X = rs.randint(-2, 3, size=(Bn, hw, hw, 3)).astype(np.float32)
    X[1, :8] = 0.0                                              # a flat region: whole windows tie (or are all zero)
    layers = C.vgg_layers(w, cfg)
    eng, side = _engine(cfg, hw, Bn, 2 * Bn, w)
    eng.set_precision(prec)
    eng.encode_images(X)
    feat = eng.get_features().cpu().numpy().reshape(Bn, side, side, -1)
    feat_ref = C.forward(layers, X)
    assert np.array_equal(feat, feat_ref.astype(np.float32))   # integers: exact
    n_tie = n_zero = 0
    # the case really contains what it is meant to test: count tied / all-zero windows in front of every pool
    inputs = C.forward(layers, X, return_inputs=True)[1]
    for a in [C._nhwc(x).numpy() for L, x in zip(layers, inputs) if L[0] == "pool"]:      # (N, H, W, C), post-ReLU
        win = a.reshape(a.shape[0], a.shape[1] // 2, 2, a.shape[2] // 2, 2, a.shape[3]).transpose(0, 1, 3, 5, 2, 4)
        win = win.reshape(win.shape[:4] + (4,))
        mx = win.max(-1, keepdims=True)
        n_tie += int((((win == mx).sum(-1) > 1) & (mx[..., 0] > 0)).sum())
        n_zero += int((mx[..., 0] == 0).sum())
    assert n_tie > 50 and n_zero > 50, (n_tie, n_zero)
    idx = [0, 1, 1, 0]
    R = (rs.standard_normal((4,) + feat_ref.shape[1:]) * (feat_ref[idx] + 1.0)).astype(np.float32)
    out = eng.cnn_explain(idx, R).cpu().numpy()
    ref = C.analyze(layers, X[idx], R)
    errs = [rel_l1(out[i], ref[i]) for i in range(4)]
    report("cnn_pool_ties_" + prec, max_rel_l1=max(errs), ties=n_tie, zero_windows=n_zero)
    assert max(errs) < 1e-5, errs
    # element for element: relevance lands on exactly the pixels the oracle routes it to
    assert np.array_equal(out != 0, ref != 0)



RAGGED_CFG = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, False), ("c4", 128, 256, True), ("c5", 256, 256, False)]


def test_compact_pool_interfaces_on_ragged_stack_tiles():
    """The compact pool interfaces (conv_igemm.h ConvArgs::up2_pairs) away from VGG16's friendly geometry: a 60 x 80 image,
    so that behind the second pool the 128 x 128 halo kernel's tiles are 9 stack rows x 14 columns on 30 x 40 maps — tiles
    straddle tokens (separator rows inside the resident image), the last column tile is ragged (12 of 14 columns) — and its
    in-loop loader builds eight channel chunks from (pairs, position bytes); behind the first pool the weights-in-registers
    kernel takes pairs into its folded launch on 60 x 80 maps (last column tile 10 of 14).  36 relevance maps over 3 images
    (enough rows for the large-tile paths), tokens interleaved, against the float64 literal graph."""
    from lrp_imagecaptioning_amd.engine import LRPEngine
    rs = np.random.RandomState(11)
    w = vgg_weights(rs, RAGGED_CFG, bias_std=0.3)
    layers = C.vgg_layers(w, RAGGED_CFG)
    B, T, H, W = 3, 12, 60, 80
    X = rs.uniform(-120, 130, size=(B, H, W, 3)).astype(np.float32)
    eng = LRPEngine(decoder="adaptive", cnn_cfg=RAGGED_CFG, img_hw=(H, W), L=(H // 4) * (W // 4), D=256, H=32, E=32, V=50,
                    max_images=B, max_tokens=B * T, max_caption_len=4)
    eng.set_weights(w)
    eng.encode_images(X)
    feat_ref = C.forward(layers, X)
    feat = eng.get_features().cpu().numpy().reshape(feat_ref.shape)
    assert rel_l1(feat, feat_ref) < 1e-5
    idx = [(3 * k + k // 5) % B for k in range(B * T)]                 # interleaved, uneven token -> image map
    R = (rs.standard_normal((B * T,) + feat_ref.shape[1:]) * feat_ref[idx]).astype(np.float32)
    R[5] = 0.0                                                          # an all-zero relevance map stays all zero
    out = eng.cnn_explain(idx, R).cpu().numpy()
    ref = C.analyze(layers, X[idx], R)
    assert np.isfinite(out).all() and not out[5].any()
    errs = [rel_l1(out[i], ref[i]) for i in range(B * T) if i != 5]
    # per image row / column too: the ragged last column tile and the separator rows are single bands of the map
    keep = [i for i in range(B * T) if i != 5]
    bar, band32 = band_bar(C.analyze(layers, X[idx], R, dtype=torch.float32)[keep], ref[keep])
    band = max(band_rel_l1(out[i], ref[i], where=True) for i in keep)
    report("cnn_ragged_compact", max_rel_l1=max(errs), worst_band=band[0], worst_band_at=band[1], f32_restatement_band=band32,
           band_bar=bar)
    assert max(errs) < TOL, errs
    assert band[0] < bar, (band, bar)
    # the same maps explained a few at a time (small grids: expanded interface, 64 x 64 tiles) agree bit for bit
    part = eng.cnn_explain(idx[:2], R[:2]).cpu().numpy()
    assert np.array_equal(part, out[:2])
