"""CPU: the restatements of the ResNet walk under a rule pair (tests/resnet_rule_ref.py) that the GPU tests of
tests/test_gpu_resnet_rules.py stand on, the conditioning of their draws, and the host-side surfaces of the pair."""
import numpy as np
import pytest

import resnet_ab_ref as AB
import resnet_rule_cases as RC
import resnet_rule_ref as RR
from conftest import rel_l1


@pytest.mark.parametrize("alpha,beta", [(1, 0), (2, 1)])
def test_alpha_beta_with_bias_twice_is_the_one_rule_walk(alpha, beta):
    w, spec, X, _, R = RC.draw("mid")
    r = RC.AB(alpha, beta)
    assert rel_l1(RR.analyze(w, spec, X, R, r, r), AB.analyze(w, spec, X, R, alpha, beta)) < 1e-12


@pytest.mark.parametrize("net", ["ident", "proj", "s64"])
@pytest.mark.parametrize("pair", sorted(RC.PAIRS) + ["a2b1/a1b0", "eps.25/a2b1-nobias"])
def test_cached_algorithm_equals_the_literal_walk(net, pair):
    """Proves the constant denominators (147, the sum of w^2, the bounded rule's per-channel constants with pad cells at low /
    high), the `- b` forms of the IgnoreBias rules and that the two records are independent (the last two pairs: a two-chain stem
    under one-chain units and the reverse)."""
    extra = {"a2b1/a1b0": (RC.AB(2, 1), RC.AB(1, 0)), "eps.25/a2b1-nobias": (RC.EPS(0.25), RC.AB(2, 1, False))}
    rs, ru = extra[pair] if pair in extra else RC.PAIRS[pair]
    w, spec, X, _, R = RC.draw(net)
    lit = RR.analyze(w, spec, X, R, rs, ru)
    err = rel_l1(RR.analyze_cached(w, spec, X, R, rs, ru), lit)
    print("%s %s: cached vs literal %.3e" % (net, pair, err))
    assert np.isfinite(lit).all() and np.abs(lit).sum() > 0
    assert err < 1e-10


@pytest.mark.parametrize("net,pair", RC.CASES, ids=["%s-%s" % c for c in RC.CASES])
def test_every_gpu_draw_is_well_conditioned(net, pair):
    """noise32 <= 3e-5: the condition every GPU parity test asserts before it compares."""
    c = RC.case(net, pair)
    print("%s %s: noise32 %.3e band32 %.3e" % (net, pair, c["noise32"], c["band32"]))
    assert c["noise32"] <= RC.NOISE_MAX


def test_caption_spec_takes_the_keywords_of_LRP_on_both_encoders():
    from lrp_imagecaptioning_amd.analyzer import rule_table
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec
    w = {"output_W": np.zeros((4, 7), np.float32)}
    rn = dict(img_encoder="resnet101", resnet={"stem": 8, "stacks": ((8, 2),)})
    s = CaptionModelSpec(w, cnn_rule={"rule": "Alpha2Beta1", "input_layer_rule": "Flat"}, **rn)
    assert s.cnn_rule is None and s.cnn_rules == (("flat",), ("alphabeta", 2, 1, True))
    s = CaptionModelSpec(w, cnn_rule={"rule": "Z"}, **rn)
    assert s.cnn_rules == (("epsilon", 0.0, True), ("epsilon", 0.0, True))
    s = CaptionModelSpec(w, cnn_rule={"rule": "ZPlus", "input_layer_rule": (-1.0, 2.0)}, **rn)
    assert s.cnn_rules == (("bounded", -1.0, 2.0), ("alphabeta", 1, 0, False))
    s = CaptionModelSpec(w, cnn_rule={"rule": "Alpha2Beta1"}, **rn)          # the one-rule entry, from either form
    assert s.cnn_rule == (2, 1) and s.cnn_rules is None
    cfg = [("c1", 3, 8, True), ("c2", 8, 8, False)]
    v = CaptionModelSpec(w, cnn_cfg=cfg, cnn_rule={"rule": "Alpha2Beta1", "input_layer_rule": "Flat"})
    assert v.cnn_rules == rule_table("Alpha2Beta1", "Flat", len(v.cnn_cfg))
    with pytest.raises(ValueError):
        CaptionModelSpec(w, cnn_rule={"input_layer_rule": "Flat"}, **rn)
    with pytest.raises(ValueError):
        CaptionModelSpec(w, cnn_rule={"rule": "Z", "epsilon": 1}, **rn)


def test_refusals_that_stay():
    from lrp_imagecaptioning_amd.analyzer import resnet_rule_pair
    from lrp_imagecaptioning_amd.explainers import CaptionModelSpec
    w = {"output_W": np.zeros((4, 7), np.float32)}
    rn = dict(img_encoder="resnet101", resnet={"stem": 8, "stacks": ((8, 2),)})
    for bad in ("presetBflat", "zplus", "z", ["Alpha2Beta1"] * 7):           # preset names and lists on a ResNet spec
        with pytest.raises(NotImplementedError, match="ResNet"):
            CaptionModelSpec(w, cnn_rule=bad, **rn)
    with pytest.raises(NotImplementedError, match="ResNet"):                 # a list inside the dict form
        CaptionModelSpec(w, cnn_rule={"rule": ["Z"] * 7}, **rn)
    with pytest.raises(NotImplementedError, match="ResNet"):
        resnet_rule_pair(["Alpha2Beta1"] * 7, "Flat")
    for above in ("Flat", "WSquare", ("bounded", -1, 1)):                    # input-layer kinds above the stem
        with pytest.raises(NotImplementedError):
            resnet_rule_pair(above)
    assert resnet_rule_pair("ZPlus", "Flat") == (("flat",), ("alphabeta", 1, 0, False))
    assert resnet_rule_pair("Epsilon") == (("epsilon", 1e-7, True), ("epsilon", 1e-7, True))
