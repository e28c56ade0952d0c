"""-m gpu: the gradient baselines on the ResNet encoder (lrp_cnn_walk, LRP_PREC_FP32) through the C ABI against the float64
autograd restatement tests/resnet_grad_ref.py (Gradient / InputTimesGradient / GuidedBackprop of innvestigate's
gradient_based.py on the ResNet-v1 graph cut at conv5_block3_out)."""
import numpy as np
import pytest
import torch

import resnet_grad_ref as RG
from conftest import rel_l1
from gpu_util import band_bar, band_rel_l1, report
from lrp_imagecaptioning_amd.synthetic import RESNET101_STACKS, resnet_weights

pytestmark = pytest.mark.gpu
TOL = 1e-4
WALKS = ("gradient", "input_x_gradient", "guided_backprop")
SMALL = [("tiny", ((4, 2), (8, 2)), 8, 32),                 # widths % 8 != 0
         ("mid", ((8, 2), (16, 3), (32, 2)), 16, 64),
         ("stem64", ((32, 2), (64, 2)), 64, 96)]           # 64-channel stem: the fused stem reverse, ragged patches


def _engine(stacks, stem, hw, B, ntok, w=None):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    side = hw // 4 // (2 ** (len(stacks) - 1))
    D = 4 * stacks[-1][0]
    eng = LRPEngine(decoder="gridtd", img_hw=(hw, hw), L=side * side, D=D, H=32, E=32, V=50, max_images=B, max_tokens=ntok,
                    max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
    if w is not None:
        eng.set_weights(w)
    eng.set_precision("fp32")
    return eng, side, D


def _case(name, seed=3, B=2):
    stacks, stem, hw = {n: (s, st, h) for n, s, st, h in SMALL}[name]
    rs = np.random.RandomState(seed)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    return rs, w, RG.resnet_spec(stacks, stem=stem), X, stacks, stem, hw


@pytest.mark.parametrize("name", [s[0] for s in SMALL])
def test_small_resnets_gradient_walks_match_oracle(name):
    from lrp_imagecaptioning_amd.engine import switches
    rs, w, spec, X, stacks, stem, hw = _case(name)
    eng, side, D = _engine(stacks, stem, hw, 2, 4, w)
    eng.encode_images(X)
    idx = [0, 1, 1, 0]                                     # heads crossing images
    head = rs.standard_normal((4, side, side, D)).astype(np.float32)
    for walk in WALKS:
        out = eng.cnn_walk(idx, head, walk).cpu().numpy()
        ref = RG.gradient_analyze(w, spec, X[idx], head, walk)
        errs = [rel_l1(out[i], ref[i]) for i in range(4)]
        # the worst single image row / column as well (gpu_util.band_rel_l1), held to 10 x the float32 oracle's own figure
        bar, band32 = band_bar(RG.gradient_analyze(w, spec, X[idx], head, walk, dtype=torch.float32), ref)
        band = max(band_rel_l1(out[i], ref[i], where=True) for i in range(4))
        report("resnet_grad_" + name, walk=walk, max_rel_l1=max(errs), worst_band=band[0], worst_band_at=band[1],
               f32_restatement_band=band32, band_bar=bar)
        assert np.isfinite(out).all()
        assert max(errs) < TOL, (walk, errs)
        assert band[0] < bar, (walk, band, bar)
        if name == "stem64":                               # the two-kernel stem (GEMM + stencil) as well
            with switches(LRP_IMG_FUSED="0"):
                out2 = eng.cnn_walk(idx, head, walk).cpu().numpy()
            errs2 = [rel_l1(out2[i], ref[i]) for i in range(4)]
            band2 = max(band_rel_l1(out2[i], ref[i], where=True) for i in range(4))
            report("resnet_grad_stem64_two_kernel", walk=walk, max_rel_l1=max(errs2), worst_band=band2[0], worst_band_at=band2[1])
            assert max(errs2) < TOL, (walk, errs2)
            assert band2[0] < bar, (walk, band2, bar)


def test_resnet101_full_size_gradient_walks():
    """ResNet-101 at 224 x 224, one image, two heads.  Through ~100 ReLU layers a few near-zero decisions flip even between
    float32 and float64, so the bar is 3x what the same restatement in float32 on the CPU is off by (and at least 1e-4)."""
    rs = np.random.RandomState(0)
    w = resnet_weights(rs)
    spec = RG.resnet_spec()
    X = rs.uniform(-120, 130, size=(1, 224, 224, 3)).astype(np.float32)
    eng, side, D = _engine(RESNET101_STACKS, 64, 224, 1, 2, w)
    eng.encode_images(X)
    head = rs.standard_normal((2, 7, 7, 2048)).astype(np.float32)
    X2 = np.repeat(X, 2, axis=0)
    for walk in WALKS:
        out = eng.cnn_walk([0, 0], head, walk).cpu().numpy()
        ref = RG.gradient_analyze(w, spec, X2, head, walk)
        ref32 = RG.gradient_analyze(w, spec, X2, head, walk, dtype=torch.float32)
        err = max(rel_l1(out[i], ref[i]) for i in range(2))
        err32 = max(rel_l1(ref32[i], ref[i]) for i in range(2))
        report("resnet101_grad", walk=walk, max_rel_l1=err, f32cpu_rel_l1=err32)
        assert np.isfinite(out).all()
        assert err <= max(TOL, 3 * err32), (walk, err, err32)


def test_gradient_walk_properties():
    rs, w, spec, X, stacks, stem, hw = _case("mid", seed=7, B=3)
    eng, side, D = _engine(stacks, stem, hw, 3, 6, w)
    h = rs.standard_normal((3, side, side, D)).astype(np.float32)
    h2 = rs.standard_normal((3, side, side, D)).astype(np.float32)
    eng.encode_images(X)
    batch = {wk: eng.cnn_walk([0, 1, 2], h, wk).clone() for wk in WALKS}
    # linearity of the gradient in the head; guided backprop is positively homogeneous, exactly for a power of two
    g1, g2 = batch["gradient"], eng.cnn_walk([0, 1, 2], h2, "gradient").clone()
    g12 = eng.cnn_walk([0, 1, 2], 0.75 * h - 2.5 * h2, "gradient")
    lin = float((g12 - (0.75 * g1 - 2.5 * g2)).abs().sum() / g12.abs().sum())
    assert lin < 1e-6, lin
    assert torch.equal(eng.cnn_walk([0, 1, 2], 2 * h, "guided_backprop"), 2 * batch["guided_backprop"])
    for wk in WALKS:
        assert (eng.cnn_walk([0, 1, 2], np.zeros_like(h), wk) == 0).all(), wk
    # an image's maps inside the batch == the image encoded alone, bit for bit
    for n in range(3):
        eng.encode_images(X[n:n + 1])
        for wk in WALKS:
            assert torch.equal(eng.cnn_walk([0], h[n:n + 1], wk), batch[wk][n:n + 1]), (n, wk)
    report("resnet_grad_properties", linearity=lin)


def test_other_modes_refuse_and_lrp_still_runs():
    rs, w, spec, X, stacks, stem, hw = _case("tiny")
    eng, side, D = _engine(stacks, stem, hw, 2, 2, w)
    head = rs.standard_normal((2, side, side, D)).astype(np.float32)
    for mode in ("bf16x3", "f16x2"):
        eng.set_precision(mode)
        eng.encode_images(X)
        for wk in WALKS:
            with pytest.raises(NotImplementedError, match="LRP_PREC_FP32"):
                eng.cnn_walk([0, 1], head, wk)
        assert np.isfinite(eng.cnn_walk([0, 1], head, "lrp").cpu().numpy()).all()
    eng.set_precision("fp32")                              # and back: a new fp32 encode records the masks again
    eng.encode_images(X)
    out = eng.cnn_walk([0, 1], head, "gradient").cpu().numpy()
    assert rel_l1(out, RG.gradient_analyze(w, spec, X, head, "gradient")) < TOL


def test_device_weights_and_reset_weights():
    rs, w, spec, X, stacks, stem, hw = _case("stem64", seed=11)
    host, side, D = _engine(stacks, stem, hw, 2, 2, w)
    dev, _, _ = _engine(stacks, stem, hw, 2, 2)
    dev.set_weights_from_device({k: torch.as_tensor(v).cuda() for k, v in w.items()})
    head = rs.standard_normal((2, side, side, D)).astype(np.float32)
    for e in (host, dev):
        e.encode_images(X)
    for wk in WALKS:
        assert torch.equal(host.cnn_walk([0, 1], head, wk), dev.cnn_walk([0, 1], head, wk)), wk
    # new weights of one unit (kernel and BN scale), from the host on one handle and from the device on the other: the
    # walk follows them (the BN-scaled gradient copy is repacked, not reused)
    w2 = dict(w)
    for k in ("conv3_block1_2_conv_W", "conv3_block1_2_bn_gamma", "conv1_conv_W", "conv1_bn_var"):
        w2[k] = (w[k] * rs.uniform(0.5, 1.5, size=w[k].shape)).astype(np.float32)
    host.set_weights({k: w2[k] for k in ("conv3_block1_2_conv_W", "conv3_block1_2_bn_gamma", "conv1_conv_W", "conv1_bn_var")})
    dev.set_weights_from_device({k: torch.as_tensor(w2[k]).cuda() for k in ("conv3_block1_2_conv_W", "conv3_block1_2_bn_gamma",
                                                                           "conv1_conv_W", "conv1_bn_var")})
    for e in (host, dev):
        e.encode_images(X)
    for wk in WALKS:
        ref = RG.gradient_analyze(w2, spec, X, head, wk)
        a, b = host.cnn_walk([0, 1], head, wk), dev.cnn_walk([0, 1], head, wk)
        assert torch.equal(a, b), wk
        err = max(rel_l1(a[i].cpu().numpy(), ref[i]) for i in range(2))
        assert err < TOL, (wk, err)
        assert rel_l1(RG.gradient_analyze(w, spec, X, head, wk), ref) > 1e-2      # (the change is visible)


def test_reference_gradient_classes_on_resnet():
    """The six baseline engines of the reference end to end on a small ResNet caption model: decoder-gradient oracle, then
    the CNN oracle (times the Grad-CAM map, upscale = image / feature side, for the guided variants)."""
    import lrp_imagecaptioning_amd.explainers as EX
    from lrp_imagecaptioning_amd.postprocess import grad_cam
    from lrp_imagecaptioning_amd.synthetic import adaptive_weights, gridtd_weights
    from oracle.decoder_grad_ref import AdaptiveGradOracle, GridTDGradOracle
    stacks, stem, hw, H, V = ((8, 2), (16, 2)), 8, 32, 32, 50
    L, D = 16, 64
    for kind in ("adaptive", "gridtd"):
        rs = np.random.RandomState(5)
        w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
        w.update((adaptive_weights if kind == "adaptive" else gridtd_weights)(rs, L, D, H, H, V))
        spec = EX.CaptionModelSpec(w, img_encoder="resnet101", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V,
                                   img_hw=(hw, hw), resnet={"stem": stem, "stacks": stacks})
        X = rs.uniform(-120, 130, size=(1, hw, hw, 3)).astype(np.float32)
        rspec = RG.resnet_spec(stacks, stem=stem)
        feat = RG.forward(w, rspec, X).astype(np.float32)
        cap = [7, 19, 3, 1]
        o = (AdaptiveGradOracle if kind == "adaptive" else GridTDGradOracle)(w, L, D, H, H)
        o.forward(feat, cap)
        names = {"adaptive": ("ExplainImgCaptioningAdaptiveAttentionGradient", "ExplainImgCaptioningAdaptiveAttentionInputTimesGradient",
                              "ExplainImgCaptioningAdaptiveAttentionGuidedGradcam"),
                 "gridtd": ("ExplainImgCaptioningGridTDGradient", "ExplainImgCaptioningGridTDGradientTimesInput",
                            "ExplainImgCaptioningGridTDGuidedGradcam")}[kind]
        for cname, mode in zip(names, WALKS):
            ex = getattr(EX, cname)(spec, None, None, max_caption_length=6)
            ex._forward_beam_search((None, X), cap)
            rel = ex._explain_sentence()
            assert len(rel) == len(cap) - 1 and rel[0].shape == (1, 4, 4, D)
            worst = 0.0
            for i, d in enumerate(rel):
                dref = o.backward(i + 1)
                assert rel_l1(d, dref) < TOL
                img = ex._explain_CNN(X, d)
                ref = RG.gradient_analyze(w, rspec, X, dref, mode)
                if mode == "guided_backprop":
                    ref = ref * grad_cam(feat, dref[0], L, D, upscale=hw // int(np.sqrt(L)))[None, ..., None]
                assert img.shape == X.shape
                worst = max(worst, rel_l1(img, ref))
            report("resnet_grad_classes", cls=cname, max_rel_l1=worst)
            assert worst < TOL, (cname, worst)


def test_gradient_analyzers():
    from lrp_imagecaptioning_amd import analyzer as A
    from lrp_imagecaptioning_amd.engine import LRPEngine
    from lrp_imagecaptioning_amd.synthetic import vgg_weights
    rs = np.random.RandomState(9)
    # VGG-style spec: the analyzers are lrp_cnn_walk in fp32, bit for bit
    cfg = [("c1", 3, 16, False), ("c2", 16, 16, True), ("c3", 16, 32, False), ("c4", 32, 32, True), ("c5", 32, 64, False)]
    wv = vgg_weights(rs, cfg, bias_std=0.05)
    Xv = rs.uniform(-120, 130, size=(2, 16, 16, 3)).astype(np.float32)
    hv = rs.standard_normal((2, 4, 4, 64)).astype(np.float32)
    eng = LRPEngine(decoder="adaptive", cnn_cfg=cfg, img_hw=(16, 16), L=16, D=64, H=8, E=8, V=4, max_images=8, max_tokens=8,
                    max_caption_len=2)
    eng.set_weights(wv)
    eng.set_precision("fp32")
    eng.encode_images(Xv)
    vspec = A.ImageModelSpec(wv, cnn_cfg=cfg, img_hw=(16, 16))
    for cls, wk in ((A.Gradient, "gradient"), (A.InputTimesGradient, "input_x_gradient"), (A.GuidedBackprop, "guided_backprop")):
        got = cls(vspec).analyze([Xv, hv])
        np.testing.assert_array_equal(got, eng.cnn_walk([0, 1], hv, wk).cpu().numpy())
    g = eng.cnn_walk([0, 1], hv, "gradient").cpu().numpy()
    np.testing.assert_array_equal(A.Gradient(vspec, postprocess="abs").analyze([Xv, hv]), np.abs(g))
    np.testing.assert_array_equal(A.InputTimesGradient(vspec, postprocess="square").analyze([Xv, hv]), Xv * np.square(g))
    # ResNet spec: against the oracle
    rs2, w, spec, X, stacks, stem, hw = _case("mid", seed=4)
    rspec = A.ImageModelSpec(w, img_hw=(hw, hw), resnet={"stem": stem, "stacks": stacks})
    head = rs2.standard_normal((2,) + rspec.output_shape()).astype(np.float32)
    for cls, wk in ((A.Gradient, "gradient"), (A.InputTimesGradient, "input_x_gradient"), (A.GuidedBackprop, "guided_backprop")):
        got = cls(rspec).analyze([X, head])
        ref = RG.gradient_analyze(w, spec, X, head, wk)
        err = max(rel_l1(got[i], ref[i]) for i in range(2))
        report("resnet_grad_analyzer", walk=wk, max_rel_l1=err)
        assert err < TOL, (wk, err)
