"""-m gpu: alpha-beta LRP with beta > 0 on the ResNet encoder (lrp_set_cnn_rule on a ResNet handle; csrc/resnet_encoder.h
explain_ab) against the float64 literal walk of tests/resnet_ab_ref.py.

The rule is ill-conditioned on some draws, mostly through BatchNorm's stabiliser: the float32 literal graph is 2e-6 ... 8e-4 from
float64 depending on the seed.  The seeds below are draws whose float32 figure stays at or under 1.7e-5 on all three images
(_literal_float32: evaluated so that it does not move with the host's thread count); every parity test first asserts
noise32 <= 3e-5, so an ill-conditioned draw fails instead of widening the bar max(1e-4, 3 x noise32) (1e-4: BASELINE's bar;
noise32 as in test_a_photograph_through_resnet101_and_gridtd)."""
import functools

import numpy as np
import pytest
import torch

import resnet_ab_ref as AB
from conftest import rel_l1
from gpu_util import band_bar, band_rel_l1, report
from lrp_imagecaptioning_amd.synthetic import gridtd_weights, resnet_weights
from oracle import resnet_lrp_ref as RN

pytestmark = pytest.mark.gpu
TOL, NOISE_MAX, B = 1e-4, 3e-5, 3

# name -> (stacks, stem, (H, W), seed, takes the pair-emitting encode in bf16x3)
NETS = {
    "ident": (((8, 2),), 8, (16, 16), 1, False),
    "proj": (((8, 1),), 8, (16, 16), 3, False),
    "mid": (((8, 2), (16, 3), (32, 2)), 16, (64, 64), 7, False),
    "stem64": (((32, 2), (64, 2)), 64, (96, 96), 7, True),
    "wide": (((64, 1), (128, 1), (256, 2), (512, 1)), 64, (160, 96), 0, True),      # H != W, ResNet-101's widths
}


def _draw(net, nonneg=False):
    stacks, stem, (h, wd), seed, _ = NETS[net]
    rs = np.random.RandomState(seed)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    if nonneg:
        w = {k: (np.abs(v) if k.endswith("_conv_W") else v) for k, v in w.items()}
    spec = RN.resnet_spec(stacks, stem=stem)
    X = rs.uniform(-120, 130, (B, h, wd, 3)).astype(np.float32)
    feat = RN.forward(w, spec, X)
    R = (rs.standard_normal(feat.shape) * feat).astype(np.float32)
    return w, spec, X, feat, R


def _literal_float32(w, spec, X, R, alpha, beta):
    """The float32 literal graph on ONE thread and torch's own conv kernels.  The figure is rounding noise of a badly conditioned
    sum, so it moves with the order of summation: with oneDNN, whose blocking follows the host's vector width and thread count,
    the `wide` draw reads 1.3e-5 on one host and 3.7e-5 on another (2.7e-5 on either with one thread); this evaluation does not
    depend on the thread count of the host (1.2e-5 / 1.6e-5 on the two)."""
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.backends.mkldnn.flags(enabled=False):
            return AB.analyze(w, spec, X, R, alpha, beta, dtype=torch.float32)
    finally:
        torch.set_num_threads(nt)


@functools.lru_cache(maxsize=None)
def _case(net, alpha=2, beta=1, nonneg=False):
    """The draw of `net`, its float64 literal heat-maps under (alpha, beta), the float32 literal graph's distance from them
    (noise32) and the band bar — computed once, shared, never written to."""
    w, spec, X, feat, R = _draw(net, nonneg)
    ref = AB.analyze(w, spec, X, R, alpha, beta)
    ref32 = _literal_float32(w, spec, X, R, alpha, beta)
    noise32 = max(rel_l1(ref32[i], ref[i]) for i in range(B))
    bar, band32 = band_bar(ref32, ref)
    return dict(w=w, spec=spec, X=X, feat=feat, R=R, ref=ref, noise32=noise32, band_bar=bar, band32=band32)


def _engine(net, w, max_images=B, max_tokens=B, decoder="adaptive", H=32, V=50):
    from lrp_imagecaptioning_amd.engine import LRPEngine
    stacks, stem, (h, wd), _, _ = NETS[net]
    d = 4 * 2 ** (len(stacks) - 1)
    eng = LRPEngine(decoder=decoder, img_hw=(h, wd), L=(h // d) * (wd // d), D=4 * stacks[-1][0], H=H, E=H, V=V, max_images=max_images,
                    max_tokens=max_tokens, max_caption_len=6, resnet={"stem": stem, "stacks": stacks})
    eng.set_weights(w)
    return eng


def _check(name, out, c, **kv):
    errs = [rel_l1(out[i], c["ref"][i]) for i in range(len(out))]
    band = max(band_rel_l1(out[i], c["ref"][i], where=True) for i in range(len(out)))
    report("resnet_ab_" + name, max_rel_l1=max(errs), noise32=c["noise32"], worst_band=band[0], worst_band_at=band[1],
           f32_restatement_band=c["band32"], band_bar=c["band_bar"], **kv)
    print("resnet_ab_%s %s: rel_l1 %s noise32 %.3e band %.3e (bar %.3e)" % (name, kv, ["%.3e" % e for e in errs], c["noise32"], band[0],
                                                                            c["band_bar"]))
    assert c["noise32"] <= NOISE_MAX, c["noise32"]
    assert np.isfinite(out).all()
    assert max(errs) < max(TOL, 3 * c["noise32"]), (errs, c["noise32"])
    assert band[0] < c["band_bar"], (band, c["band_bar"])


CASES = [(net, prec, 2, 1, True) for net in NETS for prec in ("bf16x3", "fp32")] + \
        [("mid", "bf16x3", 1.5, 0.5, True), ("mid", "fp32", 1.5, 0.5, True), ("stem64", "bf16x3", 2, 1, False)]


@pytest.mark.parametrize("net,prec,alpha,beta,emit", CASES,
                         ids=["%s-%s-%g-%g%s" % (n, p, a, b, "" if e else "-LRP_FWD_EMIT=0") for n, p, a, b, e in CASES])
def test_heat_maps_match_the_literal_walk(net, prec, alpha, beta, emit):
    """Features unchanged by the rule (vs the float64 forward), heat-maps vs the float64 literal alpha-beta walk; the last case
    with the pair-emitting forward switched off (split passes between the convs, the interleaved dual launch per unit)."""
    from lrp_imagecaptioning_amd.engine import switches
    c = _case(net, alpha, beta)
    eng = _engine(net, c["w"])
    eng.set_precision(prec)
    eng.set_cnn_rule(alpha, beta)
    with switches(**({} if emit else {"LRP_FWD_EMIT": 0})):
        eng.encode_images(c["X"])
        feat = eng.get_features().cpu().numpy().reshape(c["feat"].shape)
        out = eng.cnn_explain(list(range(B)), c["R"]).cpu().numpy()
    assert rel_l1(feat, c["feat"]) < 1e-5
    _check(net, out, c, prec=prec, alpha=alpha, beta=beta, fwd_emit=emit)


@pytest.mark.parametrize("net", sorted(NETS))
def test_which_encode_a_net_takes(net):
    """stem64 and wide run the pair-emitting encode in bf16x3 (every unit's widths qualify), ident / proj / mid the other one:
    LRP_FWD_EMIT=0 changes the features' bits exactly where the emitting forward was taken (per-image scales from bounds there,
    measured per-call maxima here)."""
    from lrp_imagecaptioning_amd.engine import switches
    w, _, X, _, _ = _draw(net)
    eng = _engine(net, w)
    eng.set_cnn_rule(2, 1)
    eng.encode_images(X)
    feat = eng.get_features().clone()
    with switches(LRP_FWD_EMIT=0):
        eng.encode_images(X)
        feat0 = eng.get_features().clone()
    assert (not torch.equal(feat, feat0)) == NETS[net][4]


@pytest.mark.parametrize("net,prec", [("stem64", "bf16x3"), ("mid", "bf16x3"), ("mid", "fp32")])
def test_rule_leaves_the_default_walk_and_the_features_alone(net, prec):
    """Features bit-identical with the rule on and off; (2, 1) then (1, 0) gives the heat-maps of a handle that never set a rule,
    bit for bit; the workspace grows with the first (2, 1) and not with the second."""
    w, _, X, _, R = _draw(net)
    fresh, eng = _engine(net, w), _engine(net, w)
    idx = list(range(B))
    for e in (fresh, eng):
        e.set_precision(prec)
    fresh.encode_images(X)
    feat0, out0 = fresh.get_features().clone(), fresh.cnn_explain(idx, R).clone()
    eng.encode_images(X)                                   # (the fp32 forward allocates its ReLU masks on the first encode)
    ws0 = eng.workspace_bytes
    eng.set_cnn_rule(2, 1)
    ws1 = eng.workspace_bytes
    assert ws1 > ws0
    with pytest.raises(RuntimeError):                      # the caches belong to the old rule
        eng.cnn_explain(idx, R)
    eng.encode_images(X)
    assert torch.equal(eng.get_features(), feat0)
    out21 = eng.cnn_explain(idx, R).clone()
    assert not torch.equal(out21, out0)
    eng.set_cnn_rule(1, 0)
    eng.encode_images(X)
    assert torch.equal(eng.get_features(), feat0)
    assert torch.equal(eng.cnn_explain(idx, R), out0)
    eng.set_cnn_rule(2, 1)
    eng.encode_images(X)
    assert torch.equal(eng.cnn_explain(idx, R), out21)
    assert eng.workspace_bytes == ws1


def test_an_image_alone_equals_the_image_in_a_batch_and_the_walk_is_linear():
    """stem64 (pair-emitting encode, per-image scales): image n alone == image n inside the batch of 3, bit for bit, under (2, 1);
    and the walk is linear in R once the gates are fixed: analyze(3 R1 - 2 R2) = 3 analyze(R1) - 2 analyze(R2) up to the rounding
    of the split-bf16 operands (the bound of test_resnet101_walk_is_linear_zero_preserving_and_reproducible), zero in -> zero out."""
    w, _, X, feat, R = _draw("stem64")
    eng, one = _engine("stem64", w, max_tokens=2 * B), _engine("stem64", w, 1, 4)
    eng.set_cnn_rule(2, 1)
    one.set_cnn_rule(2, 1)
    eng.encode_images(X)
    out = eng.cnn_explain(list(range(B)), R).clone()
    for n in range(B):
        one.encode_images(X[n:n + 1])
        assert torch.equal(one.get_features()[0], eng.get_features()[n]), n
        assert torch.equal(one.cnn_explain([0], R[n:n + 1])[0], out[n]), n
    rs = np.random.RandomState(11)
    Rb = (rs.standard_normal(feat[1].shape) * feat[1]).astype(np.float32)
    o = eng.cnn_explain([1, 1, 1, 1], np.stack([R[1], Rb, 3 * R[1] - 2 * Rb, np.zeros_like(Rb)])).cpu().numpy()
    lin = rel_l1(o[2], 3 * o[0] - 2 * o[1])
    report("resnet_ab_linearity", rel_l1=lin)
    assert lin < 2e-5
    assert (o[3] == 0).all() and np.array_equal(o[0], out[1].cpu().numpy())


@pytest.mark.parametrize("prec", ["bf16x3", "fp32"])
def test_all_non_negative_weights(prec):
    """w- = 0 everywhere: Zi = b alone, the inhibitor chain carries R Bn / b against a zero matrix — finite, and the restatement's
    heat-maps (the stem still has both branches: its input is signed)."""
    c = _case("ident", 2, 1, True)                         # (a shallow net: activations grow with every all-positive conv)
    eng = _engine("ident", c["w"])
    eng.set_precision(prec)
    eng.set_cnn_rule(2, 1)
    eng.encode_images(c["X"])
    _check("ident_nonneg", eng.cnn_explain(list(range(B)), c["R"]).cpu().numpy(), c, prec=prec)


def test_interface():
    """set_cnn_rule(2, 1) on a ResNet handle; tables stay refused; the gradient walks ignore the rule."""
    c = _case("mid")
    eng, plain = _engine("mid", c["w"]), _engine("mid", c["w"])
    eng.set_cnn_rule(2, 1)
    assert eng.cnn_rule == (2, 1)
    with pytest.raises(NotImplementedError):
        eng.set_cnn_rules([("alphabeta", 2, 1, True)] * 25)
    with pytest.raises(NotImplementedError):
        eng.set_cnn_rules([("epsilon", 0.0, True)] * 25)
    idx = list(range(B))
    outs = []
    for e in (eng, plain):
        e.set_precision("fp32")
        e.encode_images(c["X"])
        outs.append([e.cnn_walk(idx, c["R"], k).clone() for k in ("gradient", "input_x_gradient", "guided_backprop")])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not torch.equal(eng.cnn_explain(idx, c["R"]), plain.cnn_explain(idx, c["R"]))


def test_reference_surface_under_presetB():
    """ExplainImgCaptioningGridTDModel on a 'presetB' ResNet spec: _explain_CNN; analyzer.LRPSequentialPresetB / LRPAlpha2Beta1 /
    LRPAlphaBeta on a ResNet ImageModelSpec: analyze([X, R]) — the parity bar of the engine tests, on the `mid` draw."""
    from lrp_imagecaptioning_amd.analyzer import ImageModelSpec, LRPAlpha2Beta1, LRPAlphaBeta, LRPSequentialPresetB
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec, ExplainImgCaptioningGridTDModel
    c = _case("mid")
    stacks, stem, hw, _, _ = NETS["mid"]
    rn = {"stem": stem, "stacks": stacks}
    L, D, H, V = 16, 128, 32, 50
    an = LRPSequentialPresetB(ImageModelSpec(c["w"], img_hw=hw, resnet=rn), epsilon=0.01, neuron_selection_mode="replace")
    _check("mid_presetB_analyzer", an.analyze([c["X"], c["R"]]), c)
    model = ImageModelSpec(c["w"], img_hw=hw, resnet=rn)
    assert np.array_equal(LRPAlpha2Beta1(model).analyze([c["X"], c["R"]]), LRPAlphaBeta(model, alpha=2).analyze([c["X"], c["R"]]))
    w = dict(c["w"])
    w.update(gridtd_weights(np.random.RandomState(5), L, D, H, H, V))
    ex = ExplainImgCaptioningGridTDModel(
        CaptionModelSpec(w, img_encoder="resnet101", hidden_dim=H, embedding_dim=H, L=L, D=D, vocab_size=V, img_hw=hw, resnet=rn,
                         cnn_rule="presetB"), None, None, max_caption_length=5)
    assert ex._engine.cnn_rule == (2, 1)
    ex._forward_beam_search((None, c["X"][:1]), [9, 21, 1])
    out = ex._explain_CNN(c["X"][:1], c["R"][:1])
    _check("mid_presetB_explainer", np.asarray(out).reshape((1,) + c["ref"].shape[1:]), c)
