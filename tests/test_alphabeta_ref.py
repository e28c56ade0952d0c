"""CPU: the float64 restatement of the alpha-beta rule (tests/alphabeta_ref.py, RR:274-322 for general alpha, beta) that the
GPU tests of the two-chain walk are measured against, pinned by what can be known without running it on a GPU — and the
parameter rules of relevance_based/utils.py:72-129 on the constructor path that needs none."""
import numpy as np
import pytest
import torch

import alphabeta_ref as AB
from lrp_imagecaptioning_amd.synthetic import vgg_weights
from oracle import cnn_lrp_ref as C

CFG = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, False)]
RULES = ((2, 1), (1.5, 0.5))


def _net(seed, bias_std=0.3, hw=8):
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, CFG, bias_std=bias_std)
    X = rs.uniform(-120, 130, size=(2, hw, hw, 3)).astype(np.float32)
    R = rs.standard_normal((2, hw // 2, hw // 2, 16)).astype(np.float32)
    return w, X, R


def test_alpha1_beta0_is_the_oracle_bit_for_bit():
    w, X, R = _net(3)
    layers = C.vgg_layers(w, CFG)
    assert np.array_equal(AB.analyze(layers, X, R, 1, 0), C.analyze(layers, X, R))
    assert np.array_equal(AB.analyze(layers, X, R, 1, 0, torch.float32), C.analyze(layers, X, R, torch.float32))


def test_hand_computed_1x1_conv_with_mixed_signs():
    # one pixel, two inputs, two outputs:  x = (2, -1);  w[ci][co] = [[1, -2], [-3, 4]];  b = (0.5, -1);  R = (3, 5)
    x = torch.tensor([2.0, -1.0], dtype=torch.float64).view(1, 2, 1, 1)
    W = np.array([[1.0, -2.0], [-3.0, 4.0]]).reshape(1, 1, 2, 2)
    b = np.array([0.5, -1.0])
    R = torch.tensor([3.0, 5.0], dtype=torch.float64).view(1, 2, 1, 1)
    # x+ = (2, 0), x- = (0, -1);  w+ = [[1, 0], [0, 4]], w- = [[0, -2], [-3, 0]];  b+ = (0.5, 0), b- = (0, -1)
    # Z_act = x+ w+ + b+ + x- w- + b- = (2, 0) + (0.5, 0) + (3, 0) + (0, -1) = (5.5, -1)
    # Z_inh = x+ w- + b- + x- w+ + b+ = (0, -4) + (0, -1) + (0, -4) + (0.5, 0) = (0.5, -9)
    sa = np.array([3 / 5.5, 5 / -1.0])
    si = np.array([3 / 0.5, 5 / -9.0])
    act = np.array([2 * (1 * sa[0] + 0 * sa[1]), -1 * (-3 * sa[0] + 0 * sa[1])])
    inh = np.array([2 * (0 * si[0] + -2 * si[1]), -1 * (0 * si[0] + 4 * si[1])])
    for alpha, beta in RULES + ((1, 0),):
        got = AB.alphabeta_conv(x, W, b, R, alpha, beta, torch.float64).numpy().ravel()
        assert np.allclose(got, alpha * act - beta * inh, rtol=1e-14, atol=0), (alpha, beta, got)


def test_no_inhibitor_where_z_inh_is_zero():
    # nonnegative weights, zero biases, nonnegative image: x- = 0 and w- = 0, so Z_inh == 0 everywhere, SafeDivide gives
    # R / 1e-7, and every product it enters has a zero factor: inh is exactly 0 and the result alpha x the (1, 0) result per conv
    rs = np.random.RandomState(5)
    w = {k: (np.abs(v) if k.endswith("_W") else np.zeros_like(v)) for k, v in vgg_weights(rs, CFG).items()}
    X = rs.uniform(0, 130, size=(1, 8, 8, 3)).astype(np.float32)
    R = rs.standard_normal((1, 4, 4, 16)).astype(np.float32)
    layers = C.vgg_layers(w, CFG)
    base = C.analyze(layers, X, R)
    for alpha, beta in RULES:
        out = AB.analyze(layers, X, R, alpha, beta)
        assert np.allclose(out, alpha ** len(CFG) * base, rtol=1e-12, atol=0)


@pytest.mark.parametrize("rule", RULES)
def test_conservation_without_biases(rule):
    # sum act == sum R and sum inh == sum R where no bias takes relevance, so alpha - beta == 1 keeps the sum
    w, X, R = _net(11, bias_std=0.0)
    w = {k: (np.zeros_like(v) if k.endswith("_b") else v) for k, v in w.items()}
    out = AB.analyze(C.vgg_layers(w, CFG), X, R, *rule)
    for i in range(len(R)):
        assert abs(out[i].sum() - R[i].astype(np.float64).sum()) <= 1e-10 * np.abs(out[i]).sum()


def test_float32_restatement_is_close_to_float64():
    w, X, R = _net(7)
    layers = C.vgg_layers(w, CFG)
    for rule in RULES:
        r64, r32 = AB.analyze(layers, X, R, *rule), AB.analyze(layers, X, R, *rule, dtype=torch.float32)
        assert np.abs(r32 - r64).sum() / np.abs(r64).sum() < 1e-5


# ---------------------------------------------------------------- relevance_based/utils.py:72-129
def test_parameter_inference():
    from lrp_imagecaptioning_amd.analyzer import infer_alpha_beta
    assert infer_alpha_beta(2, None, "X") == (2, 1)
    assert infer_alpha_beta(None, 1, "X") == (2, 1)
    assert infer_alpha_beta(1.5, None, "X") == (1.5, 0.5)
    assert infer_alpha_beta(None, 0, "X") == (1, 0)
    assert infer_alpha_beta(3, 2, "X") == (3, 2)


@pytest.mark.parametrize("alpha,beta,text", [
    (None, None, "Neither alpha or beta were given"),
    (0.5, None, "Passed parameter alpha invalid. Expecting alpha >= 1 but was 0.5"),
    (None, -1, "Passed parameter beta invalid. Expecting beta >= 0 but was -1"),
    (2, -0.5, "Passed parameter beta invalid. Expecting beta >= 0 but was -0.5"),
    (2, 0.5, "Condition alpha - beta = 1 not fulfilled. alpha=2 ; beta=0.5 -> alpha - beta = 1.5"),
    (1, 1, "Condition alpha - beta = 1 not fulfilled. alpha=1 ; beta=1 -> alpha - beta = 0"),
])
def test_bad_parameters_raise_the_reference_texts_before_any_engine_exists(alpha, beta, text):
    from lrp_imagecaptioning_amd.analyzer import LRPAlphaBeta
    with pytest.raises(ValueError) as e:
        LRPAlphaBeta(None, alpha=alpha, beta=beta)            # (model = None: the parameters are checked first, as in the reference)
    assert str(e.value) == "Constructor call to LRPAlphaBeta : " + text


def test_ignore_bias_variants_are_not_built():
    from lrp_imagecaptioning_amd.analyzer import LRPAlphaBeta
    with pytest.raises(NotImplementedError):
        LRPAlphaBeta(None, alpha=2, beta=1, bias=False)


def test_spec_accepts_rule_names():
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec
    w = {"output_W": np.zeros((4, 6), np.float32)}
    assert CaptionModelSpec(w).cnn_rule == (1, 0)
    assert CaptionModelSpec(w, cnn_rule="alpha2beta1").cnn_rule == (2, 1)
    assert CaptionModelSpec(w, cnn_rule="alpha1beta0").cnn_rule == (1, 0)
    assert CaptionModelSpec(w, cnn_rule=(1.5, None)).cnn_rule == (1.5, 0.5)
    with pytest.raises(ValueError):
        CaptionModelSpec(w, cnn_rule="epsilon")
    with pytest.raises(ValueError):
        CaptionModelSpec(w, cnn_rule=(2, 2))
