"""CPU: the restatements of tests/gradient_family_ref.py (Philox4x32-10 known answers of Random123, Deconvnet against the
guided-backprop restatement, the path transcription) and what the new analyzer classes refuse before an engine exists."""
import numpy as np
import pytest

import gradient_family_ref as GF
import resnet_grad_ref as RG
from lrp_imagecaptioning_amd.synthetic import resnet_weights, vgg_weights
from oracle import cnn_lrp_ref as C

CFG = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, True), ("c4", 16, 16, False)]


def _hex(words):
    return " ".join("%08x" % int(v) for v in words)


@pytest.mark.parametrize("ctr,key,out", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, out):
    assert _hex(GF.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))) == out


def test_gaussian_noise_is_a_function_of_seed_row_element():
    a = GF.gaussian_noise(7, [0, 1, 2, 5], 105)
    assert a.shape == (4, 105) and np.isfinite(a).all() and np.abs(a).max() <= 5.9
    np.testing.assert_array_equal(GF.gaussian_noise(7, [5], 105)[0], a[3])
    np.testing.assert_array_equal(GF.gaussian_noise(7, [2], 9)[0], a[2, :9])             # a tail group is a prefix of the full one
    assert not np.array_equal(GF.gaussian_noise(8, [0], 105)[0], a[0])
    assert not np.array_equal(GF.gaussian_noise(7 + (1 << 32), [0], 105)[0], a[0])        # the seed's high word is part of the key
    z = GF.gaussian_noise(3, np.arange(64), 4096).ravel()
    n = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / n)


def _vgg_case(nonneg, seed=0):
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, CFG, bias_std=0.3)
    X = rs.uniform(-120, 130, size=(2, 16, 16, 3)).astype(np.float32)
    if nonneg:
        w = {k: np.abs(v) for k, v in w.items()}
        X = np.abs(X)
    layers = C.vgg_layers(w, CFG)
    head = rs.standard_normal(C.forward(layers, X).shape).astype(np.float32)
    return layers, X, head


def test_deconvnet_vgg_is_guided_backprop_when_every_relu_is_on():
    layers, X, head = _vgg_case(True)
    np.testing.assert_allclose(GF.deconvnet_vgg(layers, X, head), C.gradient_analyze(layers, X, head, "guided_backprop"), rtol=1e-12,
                               atol=0)
    layers, X, head = _vgg_case(False)
    d, g = GF.deconvnet_vgg(layers, X, head), C.gradient_analyze(layers, X, head, "guided_backprop")
    assert np.abs(d - g).sum() > 0.1 * np.abs(d).sum()


def test_deconvnet_resnet_is_guided_backprop_when_every_relu_is_on():
    stacks, stem = ((4, 2), (8, 2)), 8
    spec = RG.resnet_spec(stacks, stem=stem)
    rs = np.random.RandomState(1)
    w = resnet_weights(rs, stacks, stem=stem, bias_std=0.2)
    X = rs.uniform(-120, 130, size=(1, 32, 32, 3)).astype(np.float32)
    head = rs.standard_normal(RG.forward(w, spec, X).shape).astype(np.float32)
    d, g = GF.deconvnet_resnet(w, spec, X, head), RG.gradient_analyze(w, spec, X, head, "guided_backprop")
    assert np.abs(d - g).sum() > 0.1 * np.abs(d).sum()
    # every ReLU on: non-negative kernels and input, BN an increasing map with a non-negative shift
    wp = {}
    for k, v in w.items():
        wp[k] = np.abs(v) if k.endswith(("_conv_W", "_conv_b", "_bn_gamma", "_bn_beta")) else v
        if k.endswith("_bn_mean"):
            wp[k] = np.zeros_like(v)
    Xp = np.abs(X)
    assert (RG.forward(wp, spec, Xp) > 0).all()
    np.testing.assert_allclose(GF.deconvnet_resnet(wp, spec, Xp, head), RG.gradient_analyze(wp, spec, Xp, head, "guided_backprop"),
                               rtol=1e-12, atol=0)


def test_path_transcription():
    rs = np.random.RandomState(2)
    x = rs.standard_normal((3, 4, 5)).astype(np.float64)
    n = 4
    p = GF.python_based_augment_path(x, n, 0)
    assert p.shape == (12, 4, 5)
    for b in range(3):
        for s in range(n):
            np.testing.assert_allclose(p[b * n + s], x[b] * (1 + s / n), rtol=1e-15)       # away from the reference, s / n < 1
    ref = rs.standard_normal(x.shape)
    q = GF.python_based_augment_path(x, n, ref, standard=True)
    np.testing.assert_allclose(q[0::n], ref, atol=1e-15)
    np.testing.assert_allclose(q[1::n], ref + 0.25 * (x - ref), rtol=1e-12, atol=1e-15)
    maps = rs.standard_normal(p.shape)
    np.testing.assert_allclose(GF.python_based_reduce_path(maps, n, x, ref),
                               np.stack([maps[b * n:(b + 1) * n].mean(axis=0) for b in range(3)]) * (x - ref), rtol=1e-12)
    np.testing.assert_array_equal(GF.python_based_augment_base(x, n)[5], x[1])


def test_constructor_validation_needs_no_engine():
    from lrp_imagecaptioning_amd import analyzer as A
    rs = np.random.RandomState(0)
    spec = A.ImageModelSpec(vgg_weights(rs, CFG), cnn_cfg=CFG, img_hw=(16, 16))
    with pytest.raises(ValueError, match="augment_by_n"):
        A.SmoothGrad(spec, augment_by_n=0)
    with pytest.raises(ValueError, match="augment_by_n"):
        A.IntegratedGradients(spec, steps=2.5)
    with pytest.raises(ValueError, match="postprocess"):
        A.SmoothGrad(spec, postprocess="sqrt")
    with pytest.raises(ValueError, match="postprocess"):
        A.IntegratedGradients(spec, postprocess="sqrt")
    with pytest.raises(ValueError, match="noise_scale"):
        A.SmoothGrad(spec, noise_scale=-1)
    with pytest.raises(ValueError, match="seed"):
        A.SmoothGrad(spec, seed=-1)
    with pytest.raises(ValueError, match="path"):
        A.IntegratedGradients(spec, path="geodesic")
    with pytest.raises(ValueError, match="neuron_selection parameter is not valid"):
        A.SmoothGrad(spec, neuron_selection_mode="nope")
    with pytest.raises(NotImplementedError, match="replace"):
        A.IntegratedGradients(spec, neuron_selection_mode="index")
    with pytest.raises(NotImplementedError, match="replace"):
        A.Deconvnet(spec, neuron_selection_mode="all")
    with pytest.raises(TypeError, match="engine walk"):
        A.GaussianSmoother(object())
    with pytest.raises(TypeError, match="engine walk"):
        A.PathIntegrator("gradient")


def test_analyzers_table_has_the_reference_keys_of_what_is_built():
    from lrp_imagecaptioning_amd import analyzer as A
    assert A.analyzers["deconvnet"] is A.Deconvnet and A.analyzers["smoothgrad"] is A.SmoothGrad
    assert A.analyzers["integrated_gradients"] is A.IntegratedGradients and A.analyzers["guided_backprop"] is A.GuidedBackprop
    assert A.analyzers["gradient"] is A.Gradient and A.analyzers["input_t_gradient"] is A.InputTimesGradient
    assert A.analyzers["lrp.sequential_preset_a"] is A.LRPSequentialPresetA
    for absent in ("deep_taylor", "deep_taylor.bounded", "deep_lift", "deep_lift.wrapper", "pattern.net", "pattern.attribution",
                   "gradient.baseline", "input", "random"):
        assert absent not in A.analyzers
    assert "deconvnet" in __import__("lrp_imagecaptioning_amd.engine", fromlist=["LRPEngine"]).LRPEngine.WALKS
