"""CPU: the restatement of PatternNet / PatternAttribution (tests/pattern_ref.py) against hand-sized cases and its own identities,
the argument and refusal behaviour of the Python classes without an engine, and the conditions of the draws that
tests/test_gpu_pattern.py runs the device on (tests/pattern_cases.py)."""
import warnings

import numpy as np
import pytest
import torch

import deeplift_ref as DL
import pattern_cases as PC
import pattern_ref as PR
from lrp_imagecaptioning_amd import analyzer as A
from lrp_imagecaptioning_amd import pattern as P
from lrp_imagecaptioning_amd.synthetic import vgg_weights
from oracle import cnn_lrp_ref as C


# ------------------------------------------------------------------------------------------------------------ hand-sized fits
def test_one_channel_conv_closed_form():
    """One 1 -> 1 conv whose kernel is w at the centre tap: Y = w x, so the linear pattern is cov(X_k, x) / (w var(x)) at tap k —
    1 / w at the centre — with the population moments over all positions of all images, shifted copies zero padded."""
    rs = np.random.RandomState(0)
    w = 0.75
    W = np.zeros((3, 3, 1, 1)); W[1, 1, 0, 0] = w
    X = rs.standard_normal((4, 5, 6, 1))
    layers = [("conv", W, np.array([0.3]))]
    (A_,) = PR.fit(layers, X, "linear")
    x = X[..., 0]
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1)))
    var = (x * x).mean() - x.mean() ** 2
    for ky in range(3):
        for kx in range(3):
            s = xp[:, ky:ky + 5, kx:kx + 6]
            cov = (s * x).mean() - s.mean() * x.mean()
            assert abs(A_[ky, kx, 0, 0] - cov / (w * var)) < 1e-12, (ky, kx)
    assert abs(A_[1, 1, 0, 0] - 1 / w) < 1e-12


def test_never_firing_channel_gives_zeros():
    rs = np.random.RandomState(1)
    w = vgg_weights(rs, PC.K.TINY_CFG[:1], bias_std=0.05)
    w["c1_b"] = w["c1_b"].copy(); w["c1_b"][[2, 5]] = -1e4
    layers = C.vgg_layers(w, [PC.K.TINY_CFG[0][:3] + (False,)])
    X = rs.uniform(-120, 130, size=(2, 8, 8, 3))
    (s,) = PR.fit_sums(layers, X, "relu")
    assert s["cnt"][2] == 0 and s["cnt"][5] == 0 and s["cnt"][0] > 0
    (A_,) = PR.fit(layers, X, "relu")
    assert not A_[..., [2, 5]].any() and A_[..., 0].any()
    (An,) = PR.fit(layers, X, "relu.negative")             # the complementary mask: those two always satisfy it
    assert An[..., 2].any() and An[..., 5].any()


def test_zero_denominator_divides_by_one():
    W2d = np.array([[1.0], [-1.0]])
    cov = np.array([[2.0], [2.0]])
    A_ = PR.pattern_from_means(W2d, np.zeros((2, 1)), cov, np.zeros(1))
    assert np.array_equal(A_, cov)


@pytest.mark.parametrize("net,seed", PC.FIT_DRAWS)
def test_pattern_identity(net, seed):
    """sum_k W A = 1 for every channel whose denominator is not 0, within K 2^-23 sum |W A| (float32 patterns)"""
    d = PC.fit_draw(net, seed)
    for t in PC.FIT_TYPES:
        r = PC.fit_refs(net, seed, t)
        for L, A32, s in zip(PR.conv_entries(d["layers"]), r["patterns32"], r["sums"]):
            W2d = L[1].reshape(-1, L[1].shape[-1]).astype(np.float64)
            prod = W2d * A32.reshape(W2d.shape).astype(np.float64)
            live = np.abs(PR.compute_pattern(L[1], s)).sum((0, 1, 2)) > 0
            assert live.any()
            bound = W2d.shape[0] * 2.0 ** -23 * np.abs(prod).sum(0)
            assert (np.abs(prod.sum(0) - 1)[live] <= bound[live]).all(), (t, np.abs(prod.sum(0) - 1)[live].max())


# ------------------------------------------------------------------------------------------------------------ the walk
def test_unprojected_walk_with_w_is_the_gradient():
    d = PC.walk_draw(1)
    Xi = d["X"][list(d["idx"])]
    W = [L[1] for L in PR.conv_entries(d["layers"])]
    got = PR.walk(d["layers"], Xi, d["head"], W, attribution=False, projection=False)
    want = C.gradient_analyze(d["layers"], Xi, d["head"], "gradient")
    assert PC.rel_l1(got, want) < 1e-13


@pytest.mark.parametrize("attribution", [False, True])
def test_projection_is_a_division_by_the_row_maximum(attribution):
    r, _ = PC.walk_refs(1, attribution, False)
    p, _ = PC.walk_refs(1, attribution, True)
    mx = np.abs(r).reshape(len(r), -1).max(1)
    assert (mx > 0).all()
    assert np.abs(p - r / mx[:, None, None, None]).max() < 1e-12
    assert np.abs(np.abs(p).reshape(len(p), -1).max(1) - 1).max() < 1e-12
    if not attribution:
        assert mx.max() > 1e3                              # (unprojected, the PatternNet signal of even this small net is large)


# ------------------------------------------------------------------------------------------------------------ the classes
@pytest.fixture
def no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(A, "LRPEngine", boom)
    monkeypatch.setattr(P, "LRPEngine", boom)


def _spec(resnet=False):
    if resnet:
        from lrp_imagecaptioning_amd.synthetic import resnet_weights
        stacks = ((4, 1), (8, 1))
        return A.ImageModelSpec(resnet_weights(np.random.RandomState(0), stacks, stem=8), img_hw=(32, 32), resnet={"stem": 8, "stacks": stacks})
    return A.ImageModelSpec(vgg_weights(np.random.RandomState(0), PC.K.TINY_CFG), cnn_cfg=PC.K.TINY_CFG, img_hw=(16, 16))


@pytest.mark.parametrize("cls", ["PatternNet", "PatternAttribution"])
def test_analyzer_refusals(no_engine, cls):
    k = getattr(A, cls)
    with pytest.raises(A.NotAnalyzeableModelException, match="only well defined for conv2d/max-pooling/dense"):
        k(_spec(resnet=True))
    for sw in ("reverse_keep_tensors", "reverse_check_min_max_values", "reverse_check_finite", "reverse_clip_values", "reverse_verbose"):
        with pytest.raises(NotImplementedError, match=sw):
            k(_spec(), **{sw: True})
    with pytest.raises(ValueError, match="neuron_selection parameter is not valid"):
        k(_spec(), neuron_selection_mode="nope")
    assert "patternnet" not in A.analyzers and "pattern.net" not in A.analyzers       # reached by name, like DeepLIFT


class _FakeEngine(object):
    log = []

    def __init__(self, **kw):
        self.max_images, self.max_tokens, self.L, self.D = kw["max_images"], kw["max_tokens"], kw["L"], kw["D"]
        self.img_hw = kw["img_hw"]
        type(self).log.append(("create",))

    def __getattr__(self, name):
        def rec(*a, **k):
            type(self).log.append((name,) + tuple(x for x in a if isinstance(x, (str, bool, int))))
            if name == "get_patterns":
                return ["fitted"]
            if name == "cnn_walk":
                return torch.zeros((len(a[0]), self.img_hw[0], self.img_hw[1], 3))
        return rec


def test_analyzer_arguments_reach_the_engine(monkeypatch):
    monkeypatch.setattr(A, "LRPEngine", _FakeEngine)
    _FakeEngine.log = []
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        a = A.PatternNet(_spec(), reverse_project_bottleneck_layers=False)
    assert [str(g.message) for g in got] == ["The standard setting for 'reverse_project_bottleneck_layers' is overwritten."]
    assert ("set_pattern_projection", False) in _FakeEngine.log and ("set_precision", "fp32") in _FakeEngine.log
    X, head = np.zeros((2, 16, 16, 3), np.float32), np.zeros((2, 4, 4, 16), np.float32)
    with pytest.raises(RuntimeError, match="fit"):
        a.analyze([X, head])
    _FakeEngine.log = []
    a.fit(np.zeros((5, 16, 16, 3), np.float32), batch_size=2)
    names = [e[0] for e in _FakeEngine.log]
    assert _FakeEngine.log[0] == ("pattern_fit_begin", "relu") and names.count("pattern_fit_batch") == 3 and names[-2:] == ["pattern_fit_end", "get_patterns"]
    assert a.analyze([X, head]).shape == X.shape
    assert _FakeEngine.log[-1][0] == "cnn_walk" and _FakeEngine.log[-1][-1] == "patternnet"
    _FakeEngine.log = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # the default projection does not warn
        b = A.PatternAttribution(_spec(), patterns=[0] * 5, pattern_type="linear")
    assert ("set_pattern_projection", True) in _FakeEngine.log and "set_patterns" in [e[0] for e in _FakeEngine.log]
    b.analyze([X, head])
    assert _FakeEngine.log[-1][-1] == "pattern_attribution"
    with pytest.raises(ValueError, match="Only one pattern type allowed"):
        A.PatternNet(_spec(), pattern_type=("relu", "linear")).fit(X)


def test_pattern_computer_arguments(no_engine, monkeypatch):
    with pytest.raises(NotImplementedError, match="Not supported."):
        P.PatternComputer(_spec(), compute_layers_in_parallel=False)
    with pytest.raises(ValueError, match="unknown pattern type"):
        P.PatternComputer(_spec(), pattern_type="dummy")
    with pytest.raises(Exception, match="not supported layer"):
        P.PatternComputer(_spec(resnet=True))
    pc = P.PatternComputer(_spec(), pattern_type=["linear", "relu.negative"])       # no engine before compute
    with pytest.raises(ValueError, match="one epoch"):
        pc.compute_generator([], epochs=2)
    monkeypatch.setattr(P, "LRPEngine", _FakeEngine)
    _FakeEngine.log = []
    out = pc.compute(np.zeros((3, 16, 16, 3), np.float32), batch_size=2)
    assert out == {"linear": ["fitted"], "relu.negative": ["fitted"]}
    assert [e for e in _FakeEngine.log if e[0] == "pattern_fit_begin"] == [("pattern_fit_begin", "linear"), ("pattern_fit_begin", "relu.negative")]
    assert P.PatternComputer(_spec(), pattern_type="relu").compute(np.zeros((1, 16, 16, 3), np.float32)) == ["fitted"]


# ------------------------------------------------------------------------------------------------------------ draw conditions
@pytest.mark.parametrize("net,seed", PC.FIT_DRAWS)
def test_fit_draw_conditions(net, seed):
    """The forward is exact, so every mask is the same in any arithmetic; the float32 running-means fit is within 1e-5 relative
    L1 of the float64 one per layer and type."""
    d = PC.fit_draw(net, seed)
    assert DL.forward_is_exact(d["layers"], d["X"])
    for t in PC.FIT_TYPES:
        r = PC.fit_refs(net, seed, t)
        errs = [PC.rel_l1(a32, a64) for a32, a64 in zip(r["patterns32"], r["patterns"])]
        print("pattern fit draw %s/%d %s: float32 restatement %s" % (net, seed, t, ["%.2e" % e for e in errs]))
        assert max(errs) < 1e-5, (t, errs)
        for s in r["sums"]:
            assert float(s["cnt"].max()) <= s["P"] and np.array_equal(s["cnt"], np.round(s["cnt"]))


@pytest.mark.parametrize("seed", PC.WALK_SEEDS)
def test_walk_draw_conditions(seed):
    """the float32 walk is within 3e-5 (the project's noise ceiling) of float64 in all four forms, and the float32 relu fit of
    the draw's fit images within 1e-5 of the float64 fit"""
    d = PC.walk_draw(seed)
    fit = max(PC.rel_l1(a, b) for a, b in zip(d["fit32"], d["fit64"]))
    print("pattern walk draw %d: float32 relu fit %.2e" % (seed, fit))
    assert fit < 1e-5, fit
    for attribution in (False, True):
        for projection in (False, True):
            r64, r32 = PC.walk_refs(seed, attribution, projection)
            noise = max(PC.rel_l1(r32[i], r64[i]) for i in range(len(r64)))
            print("pattern walk draw %d attribution=%s projection=%s: float32 restatement %.2e" % (seed, attribution, projection, noise))
            assert np.isfinite(r64).all() and noise < 3e-5, noise
