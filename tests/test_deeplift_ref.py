"""CPU: the DeepLIFT / DeepTaylor restatements of tests/deeplift_ref.py — hand-computed cases of the literal form, literal versus the
cached (device) form, the exactness property of the dyadic recipe, and the argument checks of the new analyzer classes, which are
raised before any engine is created."""
import numpy as np
import pytest
import torch

import deeplift_ref as DL
import rule_table_ref as RT
from conftest import rel_l1
from lrp_imagecaptioning_amd import analyzer as A
from lrp_imagecaptioning_amd.synthetic import vgg_weights
from oracle import cnn_lrp_ref as C

CFG = [("c1", 3, 16, False), ("c2", 16, 16, True), ("c3", 16, 32, False), ("c4", 32, 32, True), ("c5", 32, 64, False)]


def _centre(m):
    """a 3x3 HWIO kernel whose centre tap is the (cin, cout) matrix m: on a 1 x 1 image the conv IS that matrix"""
    m = np.asarray(m, dtype=np.float64)
    w = np.zeros((3, 3) + m.shape)
    w[1, 1] = m
    return w


def _pixel(v):
    return np.asarray(v, dtype=np.float64).reshape(1, 1, 1, -1)


# ------------------------------------------------------------------------------------------------ hand-computed cases
W2 = [[1.0, -1.0], [2.0, 1.0]]        # W[i][o]
B2 = [0.0, -1.0]


def test_one_pixel_two_inputs_two_outputs():
    """x = (2, 1), xr = (1, 0): Y = (4, 0), Yr = (1, 0), dY = (3, 0), M = (1, 0); head (6, 5) -> M A / dY = (2, 0);
    convT: (1 * 2, 2 * 2) = (2, 4); dX = (1, 1) -> (2, 4)."""
    layers = [("conv", _centre(W2), np.asarray(B2))]
    ref = _pixel([1, 0])
    for approx in (True, False):
        out = DL.deeplift_vgg(layers, _pixel([2, 1]), _pixel([6, 5]), ref, approx)
        np.testing.assert_allclose(out.ravel(), [2.0, 4.0], rtol=1e-14)


def test_zero_dx_element_with_a_live_unit_below():
    """Two layers; the first is the identity.  x = (2, 1), xr = (1, 1): the second input of layer 2 has dX = 0 on a unit that is
    alive in layer 1 (Y = Yr = 1 > 0, so also dY == 0 there).  Layer 2: Y = (4, 0), Yr = (3, 0), dY = (1, 0), head (6, 5):
    t = dX (6, 12) = (6, 0), g = (6, 12) -> switch: (6, 12); without: (6, 0).  Layer 1 (identity, dY = (1, 0) -> safe (1, 1e-7)):
    with the switch A = (6, 12): t = dX (6, 12e7) = (6, 0), g = (6, 12) -> (6, 12); without: A = (6, 0) -> (6, 0)."""
    layers = [("conv", _centre(np.eye(2)), np.zeros(2)), ("conv", _centre(W2), np.asarray(B2))]
    x, ref, head = _pixel([2, 1]), _pixel([1, 1]), _pixel([6, 5])
    np.testing.assert_allclose(DL.deeplift_vgg(layers, x, head, ref, True).ravel(), [6.0, 12.0], rtol=1e-14)
    np.testing.assert_allclose(DL.deeplift_vgg(layers, x, head, ref, False).ravel(), [6.0, 0.0], rtol=1e-14)
    np.testing.assert_allclose(DL.deeplift_vgg_cached(layers, x, [0], head, ref, True).ravel(), [6.0, 12.0], rtol=1e-14)
    np.testing.assert_allclose(DL.deeplift_vgg_cached(layers, x, [0], head, ref, False).ravel(), [6.0, 0.0], rtol=1e-14)


def test_zero_dy_on_a_live_unit_takes_the_1e7_branch():
    """W = ((1, 1), (-1, 1)), b = 0; x = (3, 1): Y = (2, 4); xr = (2, 0): Yr = (2, 2); dY = (0, 2), both alive.  Head (1, 4):
    A / safe(dY) = (1e7, 2); convT: (1e7 + 2, -1e7 + 2); dX = (1, 1)."""
    layers = [("conv", _centre([[1.0, 1.0], [-1.0, 1.0]]), np.zeros(2))]
    for approx in (True, False):
        out = DL.deeplift_vgg(layers, _pixel([3, 1]), _pixel([1, 4]), _pixel([2, 0]), approx)
        np.testing.assert_allclose(out.ravel(), [1e7 + 2, -1e7 + 2], rtol=1e-12)
    assert DL.deeplift_stats(layers, _pixel([3, 1]), _pixel([2, 0])) == [0.5]


def test_pool_routes_to_the_images_arg_max_not_the_references():
    """One channel, identity conv, 2 x 2 image, pool.  Y = ((4, 1), (2, 3)): arg-max (0, 0).  Yr = ((1, 1), (1, 5)): ITS arg-max is
    (1, 1).  Head 10 goes to (0, 0); there dY = 4 - 1 = 3 (the reference at the same cell, not its pooled 5) and dX = 3: 10."""
    layers = [("conv", _centre([[1.0]]), np.zeros(1)), ("pool",)]
    x = np.asarray([[4.0, 1.0], [2.0, 3.0]]).reshape(1, 2, 2, 1)
    ref = np.asarray([[1.0, 1.0], [1.0, 5.0]]).reshape(1, 2, 2, 1)
    head = np.full((1, 1, 1, 1), 10.0)
    want = np.asarray([[10.0, 0.0], [0.0, 0.0]]).reshape(1, 2, 2, 1)
    np.testing.assert_allclose(DL.deeplift_vgg(layers, x, head, ref, True), want, rtol=1e-14)
    np.testing.assert_allclose(DL.deeplift_vgg_cached(layers, x, [0], head, ref, True), want, rtol=1e-14)


# ------------------------------------------------------------------------------------------------ literal == cached
def _draw(seed, dyadic, patch):
    rs = np.random.RandomState(seed)
    if dyadic:
        w = DL.dyadic_vgg_weights(rs, CFG)
        X = rs.randint(-4, 5, size=(3, 16, 16, 3)).astype(np.float32)
    else:
        w = vgg_weights(rs, CFG, bias_std=0.05)
        X = rs.uniform(-120, 130, size=(3, 16, 16, 3)).astype(np.float32)
    idx = [0, 1, 2, 2, 0, 1]
    head = rs.standard_normal((6, 4, 4, 64)).astype(np.float32)
    if patch:                                              # a reference equal to image 0 outside a 6 x 6 patch
        ref = X[:1].copy()
        ref[0, 5:11, 5:11] = rs.randint(-4, 5, size=(6, 6, 3)) if dyadic else rs.uniform(-120, 130, size=(6, 6, 3))
    else:
        ref = 1.0
    return C.vgg_layers(w, CFG), X, idx, head, ref


@pytest.mark.parametrize("dyadic", [True, False])
@pytest.mark.parametrize("patch", [False, True])
@pytest.mark.parametrize("approx", [True, False])
def test_literal_equals_cached(dyadic, patch, approx):
    layers, X, idx, head, ref = _draw(3, dyadic, patch)
    lit = DL.deeplift_vgg(layers, X[idx], head, ref, approx)
    cached = DL.deeplift_vgg_cached(layers, X, idx, head, ref, approx)
    assert np.isfinite(lit).all()
    assert max(rel_l1(cached[i], lit[i]) for i in range(len(idx))) <= 1e-12


# ------------------------------------------------------------------------------------------------ the dyadic recipe
def test_dyadic_recipe_is_exact_in_float32():
    for seed in range(4):
        layers, X, idx, head, ref = _draw(seed, True, True)
        assert DL.forward_is_exact(layers, X)
        assert DL.forward_is_exact(layers, np.asarray(ref, dtype=np.float32))
        w = layers[0][1]
        assert set(np.unique(np.abs(w))) <= {0.0, 2.0 ** -round(np.log2(np.sqrt(9 * 3 * 0.25)))}
        lit = DL.deeplift_vgg(layers, X[idx], head, ref, True)
        l32 = DL.deeplift_vgg(layers, X[idx], head, ref, True, dtype=torch.float32)
        assert max(rel_l1(l32[i], lit[i]) for i in range(len(idx))) <= 3e-5


def test_a_finer_grid_loses_the_exactness():
    """the property belongs to the recipe, not to any small net: images in sixteenths and |k| <= 3 break it"""
    rs = np.random.RandomState(0)
    w = DL.dyadic_vgg_weights(rs, CFG)
    for name, _, _, _ in CFG:
        w[name + "_W"] = w[name + "_W"] * rs.randint(1, 4, size=w[name + "_W"].shape).astype(np.float32)
    X = (rs.randint(-64, 65, size=(3, 16, 16, 3)) / 16.0).astype(np.float32)
    assert not DL.forward_is_exact(C.vgg_layers(w, CFG), X)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(A, "LRPEngine", boom)


def _spec(resnet=False):
    if resnet:
        from lrp_imagecaptioning_amd.synthetic import resnet_weights
        stacks = ((4, 1), (8, 1))
        return A.ImageModelSpec(resnet_weights(np.random.RandomState(0), stacks, stem=8), img_hw=(32, 32), resnet={"stem": 8, "stacks": stacks})
    return A.ImageModelSpec(vgg_weights(np.random.RandomState(0), CFG), cnn_cfg=CFG, img_hw=(16, 16))


def test_deeplift_argument_checks(no_engine):
    spec = _spec()
    with pytest.raises(ValueError):
        A.DeepLIFT(spec, neuron_selection_mode="bogus")
    with pytest.raises(NotImplementedError):
        A.DeepLIFT(spec, neuron_selection_mode="index")
    with pytest.raises(ValueError):
        A.DeepLIFT(spec, reference_inputs="zero")
    with pytest.raises(ValueError):
        A.DeepLIFT(spec, reference_inputs=np.zeros((3, 16, 16, 3)))      # one reference per image: the reference shares ONE
    with pytest.raises(ValueError):
        A.DeepLIFT(spec, reference_inputs=float("nan"))
    with pytest.raises(NotImplementedError):
        A.DeepLIFT(_spec(resnet=True))
    with pytest.raises(ImportError):
        A.DeepLIFTWrapper(spec)
    with pytest.raises(AssertionError):                                  # every argument is fine: now the engine is asked for
        A.DeepLIFT(spec, reference_inputs=np.zeros((16, 16, 3)), approximate_gradient=False)


def test_deeptaylor_argument_checks(no_engine):
    spec = _spec()
    with pytest.raises(ValueError):
        A.BoundedDeepTaylor(spec)
    with pytest.raises(ValueError):
        A.BoundedDeepTaylor(spec, low=1.0)
    with pytest.raises(ValueError):
        A.BoundedDeepTaylor(spec, low=1.0, high=-1.0)
    with pytest.raises(NotImplementedError):
        A.DeepTaylor(_spec(resnet=True))
    with pytest.raises(NotImplementedError):
        A.BoundedDeepTaylor(_spec(resnet=True), low=-1.0, high=1.0)
    with pytest.raises(NotImplementedError):
        A.DeepTaylor(spec, neuron_selection_mode="index")
    with pytest.raises(AssertionError):
        A.DeepTaylor(spec)


def test_new_classes_are_reached_by_name_not_by_key():
    for name in ("DeepLIFT", "DeepLIFTWrapper", "DeepTaylor", "BoundedDeepTaylor"):
        assert getattr(A, name) not in A.analyzers.values()
    wrapped = A.DeepLIFT.__new__(A.DeepLIFT)
    with pytest.raises(TypeError):
        A._engine_walk(wrapped)


# ------------------------------------------------------------------------------------------------ DeepTaylor
def test_deeptaylor_is_the_default_walk_behind_the_output_relu():
    """The literal graph equals alpha1beta0 with bias on every conv (oracle.cnn_lrp_ref.analyze) and, bounded, the table
    ("Alpha1Beta0", input_layer_rule=(low, high)) — on the head as it leaves the output ReLU's gradient mapping, head [feat > 0]:
    the classes apply that mask.  It is not a no-op: the top layer's rule has no gate (its S is R / Z+), so an unmasked head
    leaves relevance on dead top units."""
    rs = np.random.RandomState(11)
    w = vgg_weights(rs, CFG, bias_std=0.05)
    layers = C.vgg_layers(w, CFG)
    X = rs.uniform(-120, 130, size=(2, 16, 16, 3)).astype(np.float32)
    head = rs.standard_normal((2, 4, 4, 64)).astype(np.float32)
    feat = C.forward(layers, X)
    assert 0.05 < (feat <= 0).mean() < 0.95
    masked = head * (feat > 0)
    lit = DL.deeptaylor_vgg(layers, X, head)
    ref = C.analyze(layers, X, masked)
    assert max(rel_l1(lit[i], ref[i]) for i in range(2)) <= 1e-12
    assert min(rel_l1(C.analyze(layers, X, head)[i], ref[i]) for i in range(2)) > 1e-3
    low, high = -130.0, 140.0
    table = [("bounded", low, high)] + [("alphabeta", 1.0, 0.0, True)] * (len(CFG) - 1)
    litb = DL.deeptaylor_vgg(layers, X, head, bounds=(low, high))
    refb = RT.analyze(layers, X, masked, table)
    assert max(rel_l1(litb[i], refb[i]) for i in range(2)) <= 1e-12
    assert A.rule_table("Alpha1Beta0", (low, high), len(CFG)) == tuple(A.normalize_rule(r) for r in table)
