"""CPU: the references of the ResNet alpha-beta walk (tests/resnet_ab_ref.py) against each other and against the alpha1beta0
oracle, relevance conservation, and the spec surface (no GPU)."""
import numpy as np
import pytest

import resnet_ab_ref as AB
from conftest import rel_l1
from lrp_imagecaptioning_amd.synthetic import resnet_conv_list, resnet_weights
from oracle import resnet_lrp_ref as RN

NETS = {"ident": (((8, 2),), 8, 16), "two_stacks": (((4, 2), (8, 2)), 8, 32)}      # identity + projection blocks, a stride-2 stack


def _draw(name, seed, B=2):
    stacks, stem, hw = NETS[name]
    rs = np.random.RandomState(seed)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    spec = RN.resnet_spec(stacks, stem=stem)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    feat = RN.forward(w, spec, X)
    R = (rs.standard_normal(feat.shape) * feat).astype(np.float32)
    return w, spec, X, R, stacks, stem


@pytest.mark.parametrize("name", sorted(NETS))
def test_literal_walk_at_alpha1_beta0_is_the_oracle(name):
    w, spec, X, R, _, _ = _draw(name, 5)
    assert rel_l1(AB.analyze(w, spec, X, R, 1, 0), RN.analyze(w, spec, X, R)) < 1e-12
    assert rel_l1(AB.analyze_cached(w, spec, X, R, 1, 0), RN.analyze_cached(w, spec, X, R)) < 1e-12


@pytest.mark.parametrize("alpha,beta", [(2, 1), (1.5, 0.5)])
@pytest.mark.parametrize("name", sorted(NETS))
def test_cached_two_chain_algorithm_equals_literal_walk(name, alpha, beta):
    """float64 both: the restructuring (cached gates, one GEMM over both chains, the full bias in both denominators) changes the
    order of float64 operations only — the bound of tests/test_oracle_resnet.py for the one-chain algorithm."""
    w, spec, X, R, _, _ = _draw(name, 1)
    lit = AB.analyze(w, spec, X, R, alpha, beta)
    assert np.isfinite(lit).all() and (lit < 0).any()
    assert rel_l1(AB.analyze_cached(w, spec, X, R, alpha, beta), lit) < 1e-10
    assert rel_l1(lit, RN.analyze(w, spec, X, R)) > 1e-2             # another rule, not alpha1beta0 again


@pytest.mark.parametrize("alpha,beta", [(1, 0), (2, 1)])
def test_relevance_is_conserved_without_biases(alpha, beta):
    """Zero conv biases and identity BatchNorm: act and inh each hand on all of R (alpha - beta = 1), Add and the pools conserve
    it, padding positions carry x = 0 — so sum R_image = sum R_feat per image, PROVIDED no unit has a denominator of exactly 0
    (a unit none of whose active inputs has a weight of one sign: that branch drops what arrives there; with c inputs per unit
    this happens at (3/4)^c of the units, 10 % at c = 8, hence the 64-wide net; asserted).  What is left are the 1e-7 stabilisers:
    BatchNorm's reverse keeps c^2 / (c^2 + 1e-7) of a unit's relevance, a loss of 1e-7 / c^2 that matters for |c| < 3e-4 only;
    with c spread over +-50 that is under 1e-5 of the units per BatchNorm, five of them in depth: 1e-4 of sum |R|."""
    stacks, stem, hw = ((64, 1),), 64, 16
    rs = np.random.RandomState(2)
    w = resnet_weights(rs, stacks, stem=stem)
    spec = RN.resnet_spec(stacks, stem=stem)
    for name, _, _, cout, _ in resnet_conv_list(stacks, stem):
        w[name + "_conv_b"] = np.zeros(cout, np.float32)
        w[name + "_bn_gamma"] = np.ones(cout, np.float32)
        w[name + "_bn_beta"] = np.zeros(cout, np.float32)
        w[name + "_bn_mean"] = np.zeros(cout, np.float32)
        w[name + "_bn_var"] = np.full(cout, 1.0 - RN.BN_EPS, np.float32)
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    assert AB.min_abs_denominator(w, spec, X) > 0
    feat = RN.forward(w, spec, X)
    R = (rs.standard_normal(feat.shape) * feat).astype(np.float32)
    out = AB.analyze(w, spec, X, R, alpha, beta)
    for i in range(len(X)):
        lost = abs(out[i].sum() - R[i].astype(np.float64).sum()) / np.abs(R[i]).astype(np.float64).sum()
        print("alpha %g beta %g image %d: |sum R_image - sum R_feat| / sum |R_feat| = %.3e" % (alpha, beta, i, lost))
        assert lost < 1e-4


def test_caption_spec_takes_the_presets_a_resnet_can_walk():
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec
    w = {"output_W": np.zeros((4, 7), np.float32)}
    rn = dict(img_encoder="resnet101", resnet={"stem": 8, "stacks": ((8, 2),)})
    s = CaptionModelSpec(w, cnn_rule="presetB", **rn)
    assert s.cnn_rule == (2, 1) and s.cnn_rules is None
    assert CaptionModelSpec(w, cnn_rule="alpha2beta1", **rn).cnn_rule == (2, 1)
    assert CaptionModelSpec(w, cnn_rule=(2, 1), **rn).cnn_rule == (2, 1)
    assert CaptionModelSpec(w, cnn_rule="presetA", **rn).cnn_rule == (1, 0)
    for bad in ("presetBflat", "zplus", "z", ["Alpha2Beta1"] * 7):
        with pytest.raises(NotImplementedError, match="ResNet"):
            CaptionModelSpec(w, cnn_rule=bad, **rn)
